"""Host-side mirror of the reference's model API for the scoring hot path.

Same class names, method names, argument meaning and error behaviour as the reference
(kge/model/kge_model.py, kge/model/embedder/lookup_embedder.py, complex.py, distmult.py,
transe.py, rotate.py), with every score_* routed to the fused HIP kernels.  The reference
package itself cannot travel to the GPU box, so these classes are self-contained
torch.nn.Modules; `kge_amd.libkge_plugin` wraps the same kernels in subclasses of the
*reference's* KgeModel for use inside LibKGE (modules: [..., kge_amd.libkge_plugin]).

Parameter names/shapes equal the reference's (`_entity_embedder._embeddings.weight` [E,d],
`_relation_embedder._embeddings.weight` [R,d_r]) so state_dicts / checkpoints interoperate.
"""
import math

import torch
from torch import Tensor

from . import engine


class LookupEmbedder(torch.nn.Module):
    """kge/model/embedder/lookup_embedder.py:13-112 (table owner; dropout; normalize)."""

    def __init__(self, vocab_size: int, dim: int, dropout: float = 0.0, normalize_p: float = -1.0,
                 initialize: str = "normal_", initialize_args=None, sparse: bool = False,
                 dtype=torch.float32, device=None):
        super().__init__()
        self.vocab_size, self.dim = vocab_size, dim
        self.normalize_p = normalize_p
        self._embeddings = torch.nn.Embedding(vocab_size, dim, sparse=sparse, device=device, dtype=dtype)
        getattr(torch.nn.init, initialize)(self._embeddings.weight.data, **(initialize_args or {}))
        self._normalize_embeddings()
        self.dropout = torch.nn.Dropout(max(0.0, dropout))

    def _normalize_embeddings(self):
        if self.normalize_p > 0:
            with torch.no_grad():
                self._embeddings.weight.data = torch.nn.functional.normalize(
                    self._embeddings.weight.data, p=self.normalize_p, dim=-1)

    def embed(self, indexes: Tensor) -> Tensor:
        return self._postprocess(self._embeddings(indexes.long()))

    def embed_all(self) -> Tensor:
        # the reference gathers arange(E): a full-table copy (lookup_embedder.py:107-112);
        # the weight itself is returned here, the fused kernels read it in place.
        return self._postprocess(self._embeddings.weight)

    def _postprocess(self, embeddings: Tensor) -> Tensor:
        if self.dropout.p > 0:
            embeddings = self.dropout(embeddings)
        return embeddings

    @property
    def weight(self) -> Tensor:
        return self._embeddings.weight

    def fused_ok(self) -> bool:
        """Fused gather is valid when the embedder is a pure lookup (no active dropout)."""
        return not (self.training and self.dropout.p > 0)


class RelationalScorer(torch.nn.Module):
    """kge/model/kge_model.py:111-213: embedding-level scoring, combine in spo/sp_/_po/s_o."""

    name = None

    def __init__(self, l_norm: float = 1.0):
        super().__init__()
        self._norm = float(l_norm)

    def score_emb_spo(self, s_emb: Tensor, p_emb: Tensor, o_emb: Tensor) -> Tensor:
        return self.score_emb(s_emb, p_emb, o_emb, "spo")

    def score_emb(self, s_emb: Tensor, p_emb: Tensor, o_emb: Tensor, combine: str) -> Tensor:
        n = p_emb.size(0)
        if combine in ("spo", "sp_", "_po"):
            if combine == "spo":
                assert s_emb.size(0) == n and o_emb.size(0) == n
            return _ScoreEmb.apply(self.name, combine, self._norm, s_emb, p_emb, o_emb).view(n, -1)
        if combine == "s_o":  # generic fallback of the reference (kge_model.py:202-209)
            n = s_emb.size(0)
            assert o_emb.size(0) == n
            n_p = p_emb.size(0)
            s_embs = s_emb.repeat_interleave(n_p, 0)
            p_embs = p_emb.repeat((n, 1))
            o_embs = o_emb.repeat_interleave(n_p, 0)
            return _ScoreEmb.apply(self.name, "spo", self._norm, s_embs, p_embs, o_embs).view(n, -1)
        raise ValueError('cannot handle combine="{}"'.format(combine))


class ComplExScorer(RelationalScorer):
    name = "complex"


class DistMultScorer(RelationalScorer):
    name = "distmult"


class TransEScorer(RelationalScorer):
    name = "transe"


class RotatEScorer(RelationalScorer):
    name = "rotate"


class TransHScorer(RelationalScorer):
    """kge/model/transh.py:11-78 on torch operations: the path of dense embeddings (dropout in training mode, CPU
    parameters).  The index-level calls of the TransH model run the fused kernels (csrc/transh.hip), which never build
    the [m, n, d] tensor this form needs for sp_ and _po; kge_score_emb has no TransH kernel."""

    name = "transh"

    @staticmethod
    def _project(emb: Tensor, norm_vec: Tensor) -> Tensor:
        w = torch.nn.functional.normalize(norm_vec, p=2, dim=-1)
        return emb - torch.sum(emb * w, dim=-1, keepdim=True) * w

    def score_emb(self, s_emb: Tensor, p_emb: Tensor, o_emb: Tensor, combine: str) -> Tensor:
        rel, w = torch.chunk(p_emb, 2, dim=1)  # [d_r | w_r]
        n = p_emb.size(0)
        dist = torch.nn.functional.pairwise_distance
        if combine == "spo":
            assert s_emb.size(0) == n and o_emb.size(0) == n
            out = -dist(self._project(s_emb, w) + rel, self._project(o_emb, w), p=self._norm)
        elif combine == "sp_":
            m = o_emb.size(0)
            q = (self._project(s_emb, w) + rel).repeat(m, 1)                      # [m n, d], row j n + i = query i
            t = self._project(o_emb.repeat_interleave(n, 0), w.repeat(m, 1))     # target j on relation i's hyperplane
            out = -dist(q, t, p=self._norm).view(m, n).transpose(0, 1)
        elif combine == "_po":
            m = s_emb.size(0)
            q = (self._project(o_emb, w) - rel).repeat(m, 1)
            t = self._project(s_emb.repeat_interleave(n, 0), w.repeat(m, 1))
            out = -dist(q, t, p=self._norm).view(m, n).transpose(0, 1)
        elif combine == "s_o":  # the reference's generic fallback (kge_model.py:202-209) on the spo form above
            ns = s_emb.size(0)
            assert o_emb.size(0) == ns
            return self.score_emb(s_emb.repeat_interleave(n, 0), p_emb.repeat((ns, 1)), o_emb.repeat_interleave(n, 0),
                                  "spo").view(ns, -1)
        else:
            raise ValueError('cannot handle combine="{}"'.format(combine))
        return out.reshape(n, -1)


class RescalScorer(RelationalScorer):
    """kge/model/rescal.py:14-52 on torch operations: the path of dense embeddings (dropout in training mode, CPU
    parameters).  A relation row is the mixing matrix M, row-major d x d; the index-level calls of the Rescal model run
    the fused kernels (csrc/rescal.hip); kge_score_emb has no RESCAL kernel."""

    name = "rescal"

    def score_emb(self, s_emb: Tensor, p_emb: Tensor, o_emb: Tensor, combine: str) -> Tensor:
        n, d = p_emb.size(0), s_emb.size(-1)
        mix = p_emb.view(-1, d, d)
        if combine == "spo":
            assert s_emb.size(0) == n and o_emb.size(0) == n
            out = (s_emb.unsqueeze(1).bmm(mix).view(n, d) * o_emb).sum(dim=-1)
        elif combine == "sp_":
            out = s_emb.unsqueeze(1).bmm(mix).view(n, d).mm(o_emb.transpose(0, 1))
        elif combine == "_po":
            out = mix.bmm(o_emb.unsqueeze(2)).view(n, d).mm(s_emb.transpose(0, 1))
        elif combine == "s_o":  # the reference's generic fallback (kge_model.py:202-209) on the spo form above
            ns = s_emb.size(0)
            assert o_emb.size(0) == ns
            return self.score_emb(s_emb.repeat_interleave(n, 0), p_emb.repeat((ns, 1)), o_emb.repeat_interleave(n, 0),
                                  "spo").view(ns, -1)
        else:
            raise ValueError('cannot handle combine="{}"'.format(combine))
        return out.view(n, -1)


# scorers whose predictions, shared samples and evaluation take the composed paths (no kge_topk / kge_score_neg_shared /
# fused-loss kernel behind them)
_COMPOSED_ONLY = ("transh", "rescal", "conve")


class KgeModel(torch.nn.Module):
    """Index-level API of kge/model/kge_model.py:587-789 on the fused kernels."""

    scorer_cls = None

    def __init__(self, num_entities: int, num_relations: int, dim: int, l_norm: float = 1.0,
                 dtype=torch.float32, device=None, entity_args=None, relation_args=None,
                 score_dtype=None, fused_dist_loss: bool = False, fused_f32_loss: bool = False, scorer_args=None,
                 fused_dropout: bool = False):
        super().__init__()
        # fused_dropout=True (ComplEx / DistMult / TransE / RotatE, float32 parameters on a GPU, dim <= 1024): in training
        # mode with embedder dropout, score_spo and score_neg stay on the fused kernels -- the masks are computed inside
        # them (kge_score_spo_dropout / kge_score_neg_dropout and their backward) from `dropout_seed` (taken from
        # torch.initial_seed() here; settable) and a host call counter; off by default
        self.fused_dropout = bool(fused_dropout)
        self._dropout_clock = DropoutClock()
        # fused_f32_loss=True (ComplEx / DistMult, float32 parameters on a GPU scored in float32, dim % 8 == 0): loss_sp /
        # loss_po / loss_sp_po / loss_sp_po_sum without an [n, E] matrix (kge_ce_f32_fwd / _bwd), and kl_loss_sp /
        # kl_loss_po / bce_loss_sp / bce_loss_po with or without label smoothing (kge_kl_f32_* / kge_bce_f32_*); off by
        # default
        self.fused_f32_loss = bool(fused_f32_loss)
        # fused_dist_loss=True (TransE / RotatE, float32 parameters on a GPU, l_norm 1 or 2): loss_sp / loss_po /
        # loss_sp_po / loss_sp_po_sum without an [n, E] matrix (kge_ce_dist_fwd / _bwd), and kl_loss_sp / kl_loss_po /
        # bce_loss_sp / bce_loss_po without label smoothing (kge_kl_dist_* / kge_bce_dist_*); off by default
        self.fused_dist_loss = bool(fused_dist_loss)
        # score_dtype=torch.bfloat16 with f32 parameters (ComplEx / DistMult): sp_/_po scores from
        # the bf16 matrix-core kernel on bf16 copies of the tables, gradients w.r.t. the f32 masters
        self._shadow = BF16Shadow() if (score_dtype == torch.bfloat16 and dtype == torch.float32 and
                                        self.scorer_cls in (ComplExScorer, DistMultScorer)) else None
        rel_dim = dim // 2 if self.scorer_cls is RotatEScorer else dim
        if self.scorer_cls is TransHScorer:
            rel_dim = 2 * dim  # [d_r | w_r]: transh.yaml's relation_embedder.dim: -1 (transh.py:88-94)
            if fused_dist_loss:  # no TransH kernel behind kge_ce_dist_* / kge_kl_dist_* / kge_bce_dist_*
                raise ValueError("TransH: fused_dist_loss is not supported (the losses are composed from score_sp / "
                                 "score_po)")
            if float(l_norm) not in (1.0, 2.0):
                raise ValueError("TransH: l_norm must be 1 or 2 (got {})".format(l_norm))
        if self.scorer_cls is RescalScorer:
            rel_dim = dim * dim  # M_p: rescal.yaml's relation_embedder.dim: -1 (rescal.py:78-95)
            for opt, on in (("fused_dist_loss", fused_dist_loss), ("fused_f32_loss", fused_f32_loss)):
                if on:  # no RESCAL kernel behind the fused losses
                    raise ValueError("Rescal: {} is not supported (the losses are composed from score_sp / "
                                     "score_po)".format(opt))
            if dim > engine.RESCAL_MAX_DIM:
                raise ValueError("Rescal: dim must be at most {} (got {})".format(engine.RESCAL_MAX_DIM, dim))
        if self.scorer_cls in (RotatEScorer, ComplExScorer) and dim % 2:
            raise ValueError("{} requires embeddings of even dimensionality (got {})".format(
                type(self).__name__, dim))
        relation_args = dict(relation_args or {})
        if self.scorer_cls is RotatEScorer:  # rotate.yaml:22-26
            relation_args.setdefault("initialize", "uniform_")
            relation_args.setdefault("initialize_args", {"a": -math.pi, "b": math.pi})
        self._entity_embedder = LookupEmbedder(num_entities, dim, dtype=dtype, device=device,
                                               **(entity_args or {}))
        self._relation_embedder = self._make_relation_embedder(num_relations, rel_dim, dtype, device, relation_args)
        self._scorer = self._make_scorer(l_norm, dtype, device, scorer_args)
        self._touched_rows = None  # set_touched_rows

    def _make_scorer(self, l_norm, dtype, device, scorer_args):
        """`scorer_args`: what a subclass's constructor hands to its scorer (ConvE: the network's options)"""
        return self.scorer_cls(l_norm)

    def _make_relation_embedder(self, num_relations, rel_dim, dtype, device, relation_args):
        return LookupEmbedder(num_relations, rel_dim, dtype=dtype, device=device, **relation_args)

    def set_touched_rows(self, pair, rel_pair=None):
        """`pair` = kge_amd.optim.Adagrad.enable_touched_rows(entity table) -> (grad, bitmap), or None to switch it off:
        score_spo, score_neg, score_neg_blocks and score_so hand it to their autograd nodes, whose backward then accumulates the
        entity gradient into the persistent `grad`, marks the rows in `bitmap` and leaves the table's `.grad` None
        (DESIGN.md section 25).  Shared samples (score_neg_shared) keep the dense gradient: do not mix them with it.
        `rel_pair` = kge_amd.optim.SparseAdam.enable_touched_rows(relation table): the relation gradient goes the same
        way, the batch's `p` rows marked; None: a fresh dense relation gradient per node."""
        if pair is not None and self.scorer_cls in (TransHScorer, RescalScorer):
            raise ValueError("{}: touched_rows is not supported".format(type(self).__name__))
        if pair is None and rel_pair is not None:
            raise ValueError("{}: the relation table's touched rows need the entity table's".format(type(self).__name__))
        self._touched_rows = pair if rel_pair is None else (pair, rel_pair)

    # -- accessors (kge_model.py:649-661)
    def get_s_embedder(self):
        return self._entity_embedder

    def get_o_embedder(self):
        return self._entity_embedder

    def get_p_embedder(self):
        return self._relation_embedder

    def get_scorer(self):
        return self._scorer

    def tables(self, flags: int = 0) -> engine.Tables:
        """The tables the pair scores are computed from (the bf16 copies in mixed precision)."""
        if self._shadow is not None and flags == 0:
            return self._fwd_tables()
        return engine.Tables(self._scorer.name, self._entity_embedder.weight.detach(),
                             self._relation_embedder.weight.detach(), self._scorer._norm, flags)

    def _fwd_tables(self):
        if self._shadow is None:
            return None
        return self._shadow.tables(self._scorer.name, self._entity_embedder.weight,
                                   self._relation_embedder.weight, self._scorer._norm)

    def _fused(self) -> bool:
        return self._entity_embedder.fused_ok() and self._relation_embedder.fused_ok()

    @property
    def dropout_seed(self) -> int:
        return self._dropout_clock.seed

    @dropout_seed.setter
    def dropout_seed(self, seed: int):
        self._dropout_clock.seed = int(seed)

    def _dropout_triple(self):
        """(p_entity, p_relation) if `fused_dropout` is set and embedder dropout in training mode is what keeps `_fused()`
        from holding, on tables the dropout kernels take; else None."""
        if not self.fused_dropout or self._fused() or type(self._relation_embedder) is not LookupEmbedder:
            return None
        pe, pr = float(self._entity_embedder.dropout.p), float(self._relation_embedder.dropout.p)
        if not dropout_triple_fusable(self._scorer.name, self._entity_embedder.weight, self._relation_embedder.weight,
                                      pe, pr):
            return None
        return pe, pr

    # -- scoring
    def score_spo(self, s: Tensor, p: Tensor, o: Tensor, direction=None) -> Tensor:
        if self._fused():
            return _ScoreSPO.apply(self._scorer.name, self._scorer._norm, self._entity_embedder.weight,
                                   self._relation_embedder.weight, s, p, o, self._touched_rows)
        dp = self._dropout_triple()
        if dp is not None:
            return _ScoreSPODropout.apply(self._scorer.name, self._scorer._norm, self._entity_embedder.weight,
                                          self._relation_embedder.weight, s, p, o, self._dropout_clock.next(*dp),
                                          self._touched_rows)
        se, pe, oe = self._entity_embedder.embed(s), self._relation_embedder.embed(p), self._entity_embedder.embed(o)
        return self._scorer.score_emb(se, pe, oe, combine="spo").view(-1)

    def score_neg(self, s: Tensor, p: Tensor, o: Tensor, slot: int, neg: Tensor) -> Tensor:
        """[n, K]: score of triple i with slot (0 = s, 2 = o) replaced by neg[i, k]; equals
        BatchNegativeSample.score with implementation "triple" (kge/util/sampler.py:291-306)."""
        if self._fused() and slot in (0, 2):
            return _ScoreNeg.apply(self._scorer.name, self._scorer._norm, self._entity_embedder.weight,
                                   self._relation_embedder.weight, s, p, o, int(slot), neg, self._touched_rows)
        dp = self._dropout_triple() if slot in (0, 2) else None
        if dp is not None:
            return _ScoreNegDropout.apply(self._scorer.name, self._scorer._norm, self._entity_embedder.weight,
                                          self._relation_embedder.weight, s, p, o, int(slot), neg,
                                          self._dropout_clock.next(*dp), self._touched_rows)
        K = neg.shape[1]
        tr = [x.reshape(-1).long().repeat_interleave(K) for x in (s, p, o)]
        tr[slot] = neg.reshape(-1).long()
        return self.score_spo(tr[0], tr[1], tr[2]).view(-1, K)

    def score_neg_shared(self, s: Tensor, p: Tensor, o: Tensor, slot: int, unique: Tensor, drop: Tensor = None,
                         repeat: Tensor = None) -> Tensor:
        """[n, K]: score of triple i with slot (0 = s, 2 = o) replaced by the shared sample (unique, drop, repeat) --
        NaiveSharedNegativeSample.score / DefaultSharedNegativeSample.score (kge/util/sampler.py:428-463, 537-578);
        equals score_neg on engine.shared_samples(unique, drop, repeat, n)."""
        if self.scorer_cls is RescalScorer:  # no kge_score_neg_shared kernel, and none composed in its place
            raise ValueError("Rescal: shared negative samples (score_neg_shared) are not supported; use score_neg")
        if self._fused() and slot in (0, 2) and self._scorer.name not in _COMPOSED_ONLY and \
                neg_shared_fusable(self._entity_embedder.weight, s.numel()):
            return _ScoreNegShared.apply(self._scorer.name, self._scorer._norm, self._entity_embedder.weight,
                                         self._relation_embedder.weight, s, p, o, int(slot), unique, drop, repeat)
        return self.score_neg(s, p, o, slot, engine.shared_samples(unique, drop, repeat, s.reshape(-1).numel()))

    def score_neg_blocks(self, s: Tensor, p: Tensor, o: Tensor, neg_s: Tensor = None, neg_o: Tensor = None):
        """(positives [n], [n, K_s] scores with the subject replaced by neg_s[i, k] or None, [n, K_o] with the object
        replaced or None): score_spo + score_neg per slot as ONE autograd node (one pair of table gradients in the
        backward); composed from the single calls where the fused node does not apply."""
        ent, rel = self._entity_embedder.weight, self._relation_embedder.weight
        if self._fused() and neg_blocks_fusable(ent, rel):
            return _ScoreNegBlocks.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o, neg_s, neg_o,
                                         self._touched_rows)
        pos = self.score_spo(s, p, o)
        return (pos, None if neg_s is None else self.score_neg(s, p, o, 0, neg_s),
                None if neg_o is None else self.score_neg(s, p, o, 2, neg_o))

    # score_sp / score_po without a recorded gradient return the [:, :E] view of a matrix with sector-aligned rows
    # (engine.score_pitch) instead of a contiguous tensor: see the plugin's `padded_scores` option
    padded_scores = True

    def score_sp(self, s: Tensor, p: Tensor, o: Tensor = None) -> Tensor:
        if self._fused():
            return _ScorePairs.apply(self._scorer.name, self._scorer._norm, "sp",
                                     self._entity_embedder.weight,
                                     self._relation_embedder.weight, s, p, o, self._fwd_tables(),
                                     self.padded_scores and not torch.is_grad_enabled())
        se, pe = self._entity_embedder.embed(s), self._relation_embedder.embed(p)
        oe = self._entity_embedder.embed_all() if o is None else self._entity_embedder.embed(o)
        return self._scorer.score_emb(se, pe, oe, combine="sp_")

    def score_po(self, p: Tensor, o: Tensor, s: Tensor = None) -> Tensor:
        if self._fused():
            return _ScorePairs.apply(self._scorer.name, self._scorer._norm, "po",
                                     self._entity_embedder.weight,
                                     self._relation_embedder.weight, o, p, s, self._fwd_tables(),
                                     self.padded_scores and not torch.is_grad_enabled())
        se = self._entity_embedder.embed_all() if s is None else self._entity_embedder.embed(s)
        oe, pe = self._entity_embedder.embed(o), self._relation_embedder.embed(p)
        return self._scorer.score_emb(se, pe, oe, combine="_po")

    # -- filtered top-k link prediction (kge_topk): score_sp / score_po + the masking of _filter_and_rank + torch.topk
    def _predict(self, direction: str, a: Tensor, p: Tensor, k: int, filter_index, keep):
        with torch.no_grad():
            dev = self._entity_embedder.weight.device
            filters = predict_filters(filter_index, direction, a, p, dev)
            if self._fused() and dev.type == "cuda" and self._scorer.name not in _COMPOSED_ONLY:
                return engine.topk(self.tables(), direction, a, p, k, filters, keep)
            # CPU parameters, dropout in training mode, TransH / RESCAL (no kge_topk kernel): the same rule on the composed scores
            scores = self.score_sp(a, p) if direction == "sp_" else self.score_po(p, a)
            return topk_composed(scores, k, filters, keep)

    def predict_o(self, s: Tensor, p: Tensor, k: int, filter_index=None, keep: Tensor = None):
        """(values [n, k] float32, ids [n, k] int64): the k best objects of (s_i, p_i, ?), the known answers of
        `filter_index` (a kge_amd.eval.FilterIndex) left out except keep[i]; descending score, equal scores by
        ascending entity id, NaN as -inf, (-inf, -1) where fewer than k entities are left.  No [n, E] score matrix on
        the fused path; the same ordering rule (never torch.topk) on the composed one."""
        return self._predict("sp_", s, p, k, filter_index, keep)

    def predict_s(self, p: Tensor, o: Tensor, k: int, filter_index=None, keep: Tensor = None):
        """predict_o for the subjects of (?, p_i, o_i)."""
        return self._predict("_po", o, p, k, filter_index, keep)

    # -- 1vsAll loss: train_1vsAll.py:64-65 / 75-76 in one call
    def _ce_tables(self):
        """bf16 tables for the fused loss, or None (then the loss is composed from score_sp/_po)."""
        if not self._fused() or self._scorer.name not in ("complex", "distmult"):
            return None
        w = self._entity_embedder.weight
        t = self._fwd_tables()
        if t is None and w.dtype == torch.bfloat16:
            t = engine.Tables(self._scorer.name, w.detach(), self._relation_embedder.weight.detach())
        return t if (t is not None and w.is_cuda and engine.ce_supported(t)) else None

    def _ce_dist_tables(self):
        """float32 tables for the distance scorers' fused loss (`fused_dist_loss=True`), or None (then the loss is
        composed from score_sp / score_po): TransE / RotatE, l_norm 1 or 2, pure lookups, parameters on a GPU."""
        if not self.fused_dist_loss or not self._fused() or self._scorer.name not in ("transe", "rotate"):
            return None
        w = self._entity_embedder.weight
        if not w.is_cuda or w.dtype != torch.float32 or self._scorer._norm not in (1.0, 2.0):
            return None
        t = engine.Tables(self._scorer.name, w.detach(), self._relation_embedder.weight.detach(), self._scorer._norm)
        return t if engine.ce_dist_supported(t) else None

    def _ce_f32_tables(self):
        """float32 tables for the fused loss of ComplEx / DistMult (`fused_f32_loss=True`), or None (then the loss is
        composed from score_sp / score_po): float32 parameters scored in float32, pure lookups, on a GPU, a layout
        kge_ce_f32_workspace_bytes takes."""
        if not self.fused_f32_loss or not self._fused() or self._scorer.name not in ("complex", "distmult"):
            return None
        w = self._entity_embedder.weight
        if not w.is_cuda or w.dtype != torch.float32 or self._shadow is not None:
            return None
        t = engine.Tables(self._scorer.name, w.detach(), self._relation_embedder.weight.detach())
        return t if engine.ce_f32_supported(t) else None

    # one method per loss, the direction an argument ("sp": a = s; "po": a = o): the fused rows where a family of
    # fused_loss_rows applies, else composed from the scores
    def _weights(self):
        return self._entity_embedder.weight, self._relation_embedder.weight

    def _fused_rows(self, kind: str, direction: str, a: Tensor, p: Tensor, labels: tuple, eps: float = 0.0):
        scorer = self._scorer  # (one Module.__getattr__, not two)
        return fused_loss_rows(kind, direction, scorer.name, scorer._norm, self._weights, a, p, labels, eps,
                               self._ce_tables, self._ce_dist_tables, self._ce_f32_tables)

    def _scores(self, direction: str, a: Tensor, p: Tensor) -> Tensor:
        return self.score_sp(a, p) if direction == "sp" else self.score_po(p, a)

    def _ce_rows(self, direction: str, a: Tensor, p: Tensor, label: Tensor) -> Tensor:
        rows = self._fused_rows("ce", direction, a, p, (label,))
        if rows is None:
            rows = torch.nn.functional.cross_entropy(self._scores(direction, a, p), label.long(), reduction="none")
        return rows

    def _kl_rows(self, direction: str, a: Tensor, p: Tensor, rowptr: Tensor, col: Tensor, eps: float) -> Tensor:
        rows = self._fused_rows("kl", direction, a, p, (rowptr, col), float(eps))
        return self._kl_composed(self._scores(direction, a, p), rowptr, col, eps) if rows is None else rows

    def _bce_rows(self, direction: str, a: Tensor, p: Tensor, rowptr: Tensor, col: Tensor, offset: float,
                  eps: float) -> Tensor:
        rows = self._fused_rows("bce", direction, a, p, (rowptr, col, float(offset)), float(eps))
        return self._bce_composed(self._scores(direction, a, p), rowptr, col, offset, eps) if rows is None else rows

    def loss_sp(self, s: Tensor, p: Tensor, o: Tensor) -> Tensor:
        """Per-row cross entropy of score_sp(s, p) against the true objects o ([n]); its sum is the
        reference's `self.loss(scores_sp, triples[:, 2])` with train.loss=kl (loss.py:192-207)."""
        return self._ce_rows("sp", s, p, o)

    def loss_sp_po(self, s: Tensor, p: Tensor, o: Tensor) -> Tensor:
        """[2n]: loss_sp(s, p, o) followed by loss_po(p, o, s) -- both directions of a 1vsAll batch
        from one scoring launch and one pair of gradient products (train_1vsAll.py:64-81 sums and
        back-propagates the two separately)."""
        t = self._ce_tables()
        if t is not None:
            return _FusedCE2.apply(self._entity_embedder.weight, self._relation_embedder.weight, s, p, o, t)
        return torch.cat([self.loss_sp(s, p, o), self.loss_po(p, o, s)])

    def loss_sp_po_sum(self, s: Tensor, p: Tensor, o: Tensor, scale=None) -> Tensor:
        """0-d: scale * loss_sp_po(s, p, o).sum() -- the batch loss of TrainingJob1vsAll (train_1vsAll.py:64-82 with
        scale = 1 / batch_size) -- summed inside the loss kernels' own launches, its backward taking the upstream
        gradient and `scale` (None, a float, or a float32 device scalar) as device scalars: three launches and three
        autograd nodes fewer per step than `.sum() * scale` around loss_sp_po."""
        t = self._ce_tables()
        if t is not None:
            return _FusedCE2Sum.apply(self._entity_embedder.weight, self._relation_embedder.weight, s, p, o, t, scale)
        total = self.loss_sp_po(s, p, o).sum()
        return total if scale is None else total * scale

    def loss_po(self, p: Tensor, o: Tensor, s: Tensor) -> Tensor:
        """Per-row cross entropy of score_po(p, o) against the true subjects s."""
        return self._ce_rows("po", o, p, s)

    # -- KvsAll loss: train_KvsAll.py:274-294 with train.loss=kl
    @staticmethod
    def _kl_composed(scores: Tensor, rowptr: Tensor, col: Tensor, label_smoothing: float = 0.0) -> Tensor:
        """loss.py:208-213 row by row: KLDivLoss(log_softmax(scores), normalize(labels, p=1)); labels
        smoothed as train_KvsAll.py:260-266 does."""
        n = scores.shape[0]
        cnt = (rowptr[1:] - rowptr[:-1]).to(scores.device)
        rows = torch.repeat_interleave(torch.arange(n, device=scores.device), cnt)
        labels = torch.zeros_like(scores)
        labels[rows, col.to(scores.device).long()] = 1.0
        if label_smoothing > 0.0:
            labels = (1.0 - label_smoothing) * labels + 1.0 / labels.size(1)
        y = torch.nn.functional.normalize(labels, p=1, dim=1)
        return torch.nn.functional.kl_div(torch.log_softmax(scores, dim=1), y, reduction="none").sum(dim=1)

    def kl_loss_sp(self, s: Tensor, p: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor,
                   label_smoothing: float = 0.0) -> Tensor:
        """Per-row KL divergence of softmax(score_sp(s, p)) from the normalised multi-hot labels
        given as an int64 CSR over the rows (the known objects of each (s, p) query)."""
        return self._kl_rows("sp", s, p, lbl_rowptr, lbl_col, label_smoothing)

    def kl_loss_po(self, p: Tensor, o: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor,
                   label_smoothing: float = 0.0) -> Tensor:
        return self._kl_rows("po", o, p, lbl_rowptr, lbl_col, label_smoothing)

    def multilabel_loss_sp_po(self, kind: str, s: Tensor, p_sp: Tensor, rowptr_sp: Tensor, col_sp: Tensor, o: Tensor,
                              p_po: Tensor, rowptr_po: Tensor, col_po: Tensor, offset: float = 0.0,
                              label_smoothing: float = 0.0, sum_scale: float = None):
        """(loss rows of the sp_ queries (s, p_sp), loss rows of the _po queries (p_po, o)) of a KvsAll batch, `kind`
        "kl" or "bce": kl_loss_sp + kl_loss_po (bce_loss_sp + bce_loss_po) with ONE backward for both types where the
        fused path applies (_FusedMultiLabel2; no label smoothing), else the two per-type calls.  `sum_scale` given:
        the 0-d batch loss sum_scale * (sum of all rows) instead of the two row vectors."""
        t = self._ce_tables()
        if t is not None and label_smoothing == 0.0:
            return _FusedMultiLabel2.apply(kind, float(offset), self._entity_embedder.weight, self._relation_embedder.weight,
                                           s, p_sp, rowptr_sp, col_sp, o, p_po, rowptr_po, col_po, t, sum_scale)
        if kind == "kl":
            both = (self.kl_loss_sp(s, p_sp, rowptr_sp, col_sp, label_smoothing),
                    self.kl_loss_po(p_po, o, rowptr_po, col_po, label_smoothing))
        else:
            both = (self.bce_loss_sp(s, p_sp, rowptr_sp, col_sp, offset, label_smoothing),
                    self.bce_loss_po(p_po, o, rowptr_po, col_po, offset, label_smoothing))
        return both if sum_scale is None else (both[0].sum() + both[1].sum()) * float(sum_scale)

    # -- bce loss (train.loss: bce, loss.py:137-159 with bce_type None) on multi-hot labels
    @staticmethod
    def _bce_composed(scores: Tensor, rowptr: Tensor, col: Tensor, offset: float = 0.0,
                      label_smoothing: float = 0.0) -> Tensor:
        n = scores.shape[0]
        cnt = (rowptr[1:] - rowptr[:-1]).to(scores.device)
        rows = torch.repeat_interleave(torch.arange(n, device=scores.device), cnt)
        labels = torch.zeros_like(scores)
        labels[rows, col.to(scores.device).long()] = 1.0
        if label_smoothing > 0.0:
            labels = (1.0 - label_smoothing) * labels + 1.0 / labels.size(1)
        return torch.nn.functional.binary_cross_entropy_with_logits(scores + offset, labels,
                                                                     reduction="none").sum(dim=1)

    def bce_loss_sp(self, s: Tensor, p: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor, offset: float = 0.0,
                    label_smoothing: float = 0.0) -> Tensor:
        """Per-row sum over all entities of BCEWithLogits(score_sp(s, p) + offset, multi-hot labels)."""
        return self._bce_rows("sp", s, p, lbl_rowptr, lbl_col, offset, label_smoothing)

    def bce_loss_po(self, p: Tensor, o: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor, offset: float = 0.0,
                    label_smoothing: float = 0.0) -> Tensor:
        return self._bce_rows("po", o, p, lbl_rowptr, lbl_col, offset, label_smoothing)

    # kge_score_so behind score_so (False: always the composed path; tests and tools/score_so_probe.py compare the two)
    fused_score_so = True

    def score_so(self, s: Tensor, o: Tensor, p: Tensor = None) -> Tensor:
        """[n, R] scores of (s_i, ?, o_i) against all relations, or [n, len(p)] against the relations `p`
        (kge_model.py:727-747): kge_score_so where the lookups are plain, the parameters on a GPU and the scorer one of
        ComplEx / DistMult / TransE / RotatE; else composed as the reference does (kge_model.py:202-209)."""
        ent, rel = self._entity_embedder.weight, self._relation_embedder.weight
        if self.fused_score_so and self._fused() and score_so_fusable(self._scorer.name, ent, rel, s.numel()):
            return _ScoreSO.apply(self._scorer.name, self._scorer._norm, ent, rel, s, o, p,
                                  self._touched_rows if torch.is_grad_enabled() else None)
        se, oe = self._entity_embedder.embed(s), self._entity_embedder.embed(o)
        pe = self._relation_embedder.embed_all() if p is None else self._relation_embedder.embed(p)
        return self._scorer.score_emb(se, pe, oe, combine="s_o")

    def score_sp_po(self, s: Tensor, p: Tensor, o: Tensor, entity_subset: Tensor = None) -> Tensor:
        if self._fused() and not torch.is_grad_enabled():
            return engine.score_sp_po(self.tables(), s, p, o, entity_subset)
        return torch.cat((self.score_sp(s, p, entity_subset), self.score_po(p, o, entity_subset)), dim=1)


class ComplEx(KgeModel):
    scorer_cls = ComplExScorer


class DistMult(KgeModel):
    scorer_cls = DistMultScorer


class TransE(KgeModel):
    scorer_cls = TransEScorer


class RotatE(KgeModel):
    scorer_cls = RotatEScorer

    @torch.no_grad()
    def normalize_phases(self):
        """rotate.py:103-118: wrap phases to [-pi, pi)."""
        w = self._relation_embedder.weight.data
        w[:] = torch.remainder(w + math.pi, 2.0 * math.pi) - math.pi


class TransH(KgeModel):
    """kge/model/transh.py:81-118: relation rows [d_r | w_r] of width 2 dim; float32, l_norm 1 or 2."""
    scorer_cls = TransHScorer


class Rescal(KgeModel):
    """kge/model/rescal.py:55-95: relation rows are d x d mixing matrices (width dim * dim); float32, dim <= 256."""
    scorer_cls = RescalScorer


class Tucker3RelationEmbedder(torch.nn.Module):
    """kge/model/embedder/tucker3_relation_embedder.py (a ProjectionEmbedder, projection_embedder.py:6-46): a base
    lookup table B [R, d_r] and `projection`, a bias-free Linear(d_r, d^2) with weight W [d^2, d_r]; the embedding of
    relation p is the mixing matrix M_p = (B[p] @ W^T).view(d, d).  embed / embed_all are the torch path (dense
    embeddings: dropout in training mode, CPU parameters); the index-level calls of RelationalTucker3 run
    kge_tucker3_project."""

    def __init__(self, vocab_size: int, dim: int, base_dim: int = 100, dropout: float = 0.0, base_args=None,
                 dtype=torch.float32, device=None):
        super().__init__()
        self.vocab_size, self.dim = vocab_size, dim
        self.base_embedder = LookupEmbedder(vocab_size, base_dim, dtype=dtype, device=device, **(base_args or {}))
        self.projection = torch.nn.Linear(base_dim, dim, bias=False, device=device, dtype=dtype)
        torch.nn.init.normal_(self.projection.weight.data)  # projection_embedder.yaml: initialize: normal_
        self.dropout = torch.nn.Dropout(max(0.0, dropout))  # on the mixing matrices (tucker3_relation_embedder.yaml)

    def _embed(self, base_rows: Tensor) -> Tensor:
        out = torch.nn.functional.linear(base_rows, self.projection.weight)
        return self.dropout(out) if self.dropout.p > 0 else out

    def embed(self, indexes: Tensor) -> Tensor:
        return self._embed(self.base_embedder.embed(indexes))

    def embed_all(self) -> Tensor:
        return self._embed(self.base_embedder.embed_all())

    @property
    def weight(self) -> Tensor:
        """The projected table [R, d^2] on torch operations (what generic code reads as 'the relation table')."""
        return torch.nn.functional.linear(self.base_embedder.weight, self.projection.weight)

    def fused_ok(self) -> bool:
        return self.base_embedder.fused_ok() and not (self.training and self.dropout.p > 0)


class _Tucker3Project(torch.autograd.Function):
    """[n, d^2] = B[idx] @ W^T from kge_tucker3_project; backward = kge_tucker3_project_bwd (the two float32 gradient
    products, no float atomics) and the scatter of the row gradients into B's (index_add_; the identity for all rows)."""

    @staticmethod
    def forward(ctx, B, W, idx):
        ctx.save_for_backward(B, W)
        ctx.idx = idx
        return engine.tucker3_project(B.detach(), W.detach(), idx)

    @staticmethod
    def backward(ctx, gout):
        B, W = ctx.saved_tensors
        g_rows, g_w = engine.tucker3_project_bwd(B.detach(), W.detach(), ctx.idx, gout, ctx.needs_input_grad[0],
                                                 ctx.needs_input_grad[1])
        g_b = g_rows
        if g_rows is not None and ctx.idx is not None:
            g_b = torch.zeros_like(B)
            _scatter_rows(g_b, ctx.idx, g_rows)
        return g_b, g_w, None


def tucker3_project(B: Tensor, W: Tensor, idx=None) -> Tensor:
    """The projected rows of a Tucker3 relation embedder: the HIP kernel for float32 parameters on a GPU; CPU
    parameters take torch's linear (the reference's own operation).  Anything else on a GPU is an error."""
    if B.is_cuda:
        if B.dtype != torch.float32 or W.dtype != torch.float32:
            raise ValueError("RelationalTucker3: the projection kernel takes float32 parameters (got {})".format(B.dtype))
        return _Tucker3Project.apply(B, W, idx)
    return torch.nn.functional.linear(B if idx is None else B[idx.reshape(-1).long()], W)


class Tucker3Routes:
    """How a Tucker3 model hands its relation rows to the RESCAL paths (mixed into RelationalTucker3 here and into the
    plugin's HipRelationalTucker3, which says where B and W live: `_bw()`).  Two routes:
      "all"    project rows 0 .. R and pass p through; when R <= n, and always without a recorded gradient (the
               projected table is then cached until B or W changes) unless it exceeds projected_table_max_bytes;
      "batch"  project the batch's rows and pass p' = arange(n)."""
    project = "auto"
    projected_table_max_bytes = 1 << 30
    projections = 0  # projections of the whole table without a recorded gradient (the cache's misses)
    _proj_key, _proj_table = None, None

    def _bw(self):
        raise NotImplementedError

    def route(self, n: int, project: str = None) -> str:
        mode = project or self.project
        if mode not in ("auto", "all", "batch"):
            raise ValueError("RelationalTucker3: project is 'auto', 'all' or 'batch' (got {!r})".format(mode))
        if mode != "auto":
            return mode
        B, W = self._bw()
        if not torch.is_grad_enabled():
            table_bytes = B.shape[0] * W.shape[0] * B.element_size()
            return "all" if table_bytes <= self.projected_table_max_bytes else "batch"
        return "all" if B.shape[0] <= n else "batch"

    def projected_table(self) -> Tensor:
        """[R, d^2].  Without a recorded gradient: cached on the versions of B and W (the BF16Shadow pattern) -- an
        evaluation projects once, not once per batch and chunk.  With one: projected anew, nothing is cached."""
        B, W = self._bw()
        if torch.is_grad_enabled():
            return tucker3_project(B, W, None)
        key = (B._version, W._version, B.data_ptr(), W.data_ptr(), B.device, B.dtype)
        if key != self._proj_key:
            self._proj_table, self._proj_key = tucker3_project(B, W, None), key
            self.projections += 1
        return self._proj_table

    def _rel(self, p: Tensor, project: str = None):
        """(relation table, relation index, rows) the RESCAL paths take for the batch's relations p; rows: the table
        holds one row per query and the index is arange(n) (_ScorePairs' `rel_rows`)."""
        n = p.numel()
        if self.route(n, project) == "all":
            return self.projected_table(), p, False
        B, W = self._bw()
        return tucker3_project(B, W, p.reshape(-1)), torch.arange(n, device=B.device), True


class RelationalTucker3(Tucker3Routes, KgeModel):
    """kge/model/relational_tucker3.py: RESCAL whose mixing matrices are projected from a base relation table,
    M_p = (B[p] @ W^T).view(d, d) (Tucker3RelationEmbedder).  The projection is kge_tucker3_project; everything behind
    it is the RESCAL kernels on the projected rows (the routes: Tucker3Routes).
    `project` ("auto" | "all" | "batch", here or per call) forces a route."""
    scorer_cls = RescalScorer

    def __init__(self, num_entities: int, num_relations: int, dim: int, rel_base_dim: int = 100, project: str = "auto",
                 projected_table_max_bytes: int = 1 << 30, **kw):
        if project not in ("auto", "all", "batch"):
            raise ValueError("RelationalTucker3: project is 'auto', 'all' or 'batch' (got {!r})".format(project))
        if not 1 <= int(rel_base_dim) <= engine.TUCKER3_MAX_BASE_DIM:
            raise ValueError("RelationalTucker3: rel_base_dim must be in [1, {}] (got {})".format(
                engine.TUCKER3_MAX_BASE_DIM, rel_base_dim))
        object.__setattr__(self, "_rel_base_dim", int(rel_base_dim))
        super().__init__(num_entities, num_relations, dim, **kw)
        self.project, self.projected_table_max_bytes = project, int(projected_table_max_bytes)

    def _make_relation_embedder(self, num_relations, rel_dim, dtype, device, relation_args):
        args = dict(relation_args)
        return Tucker3RelationEmbedder(num_relations, rel_dim, self._rel_base_dim, dropout=args.pop("dropout", 0.0),
                                       base_args=args, dtype=dtype, device=device)

    def _bw(self):
        return self._relation_embedder.base_embedder.weight, self._relation_embedder.projection.weight

    def tables(self, flags: int = 0) -> engine.Tables:
        return engine.Tables("rescal", self._entity_embedder.weight.detach(), self.projected_table().detach(), 1.0, flags)

    # -- scoring: the RESCAL autograd nodes over (ent, projected rows)
    def score_spo(self, s, p, o, direction=None, project=None):
        if not self._fused():
            return super().score_spo(s, p, o, direction)
        rel, p2, rows = self._rel(p, project)
        return _ScoreSPO.apply("rescal", 1.0, self._entity_embedder.weight, rel, s, p2, o, None)

    def score_neg(self, s, p, o, slot, neg, project=None):
        if not (self._fused() and slot in (0, 2)):
            return super().score_neg(s, p, o, slot, neg)
        rel, p2, rows = self._rel(p, project)
        return _ScoreNeg.apply("rescal", 1.0, self._entity_embedder.weight, rel, s, p2, o, int(slot), neg, None)

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        raise ValueError("RelationalTucker3: shared negative samples (score_neg_shared) are not supported; use "
                         "score_neg")

    def score_neg_blocks(self, s, p, o, neg_s=None, neg_o=None, project=None):
        ent = self._entity_embedder.weight
        if self._fused() and ent.is_cuda and ent.dtype == torch.float32:
            rel, p2, rows = self._rel(p, project)
            return _ScoreNegBlocks.apply("rescal", 1.0, ent, rel, s, p2, o, neg_s, neg_o, None)
        return super().score_neg_blocks(s, p, o, neg_s, neg_o)

    def score_sp(self, s, p, o=None, project=None):
        if not self._fused():
            return super().score_sp(s, p, o)
        rel, p2, rows = self._rel(p, project)
        return _ScorePairs.apply("rescal", 1.0, "sp", self._entity_embedder.weight, rel, s, p2, o, None,
                                 self.padded_scores and not torch.is_grad_enabled(), rows)

    def score_po(self, p, o, s=None, project=None):
        if not self._fused():
            return super().score_po(p, o, s)
        rel, p2, rows = self._rel(p, project)
        return _ScorePairs.apply("rescal", 1.0, "po", self._entity_embedder.weight, rel, o, p2, s, None,
                                 self.padded_scores and not torch.is_grad_enabled(), rows)

    def score_sp_po(self, s, p, o, entity_subset=None, project=None):
        if self._fused() and not torch.is_grad_enabled():
            rel, p2, rows = self._rel(p, project)
            return engine.score_sp_po(engine.Tables("rescal", self._entity_embedder.weight.detach(), rel, 1.0), s, p2, o,
                                      entity_subset)
        return torch.cat((self.score_sp(s, p, entity_subset, project=project),
                          self.score_po(p, o, entity_subset, project=project)), dim=1)


def conve_image_shape(dim: int, aspect_ratio: float = 2, round_dim: bool = False):
    """(h, w, d) of conve.py:17-42: h = sqrt(d / aspect_ratio), w = h * aspect_ratio; round_dim rounds h up and d with
    it, otherwise a d that does not factor raises the reference's error."""
    height = math.sqrt(dim / aspect_ratio)
    width = height * aspect_ratio
    rounded = math.ceil(height)
    if round_dim and rounded != height:
        height = rounded
        width = height * aspect_ratio
        dim = height * width
    elif dim % height or dim % width:
        raise Exception(("Embedding dimension {} incompatible with aspect ratio {}; width ({}) or height ({}) is not "
                         "integer. Adapt dimension or set conve.round_dim=true").format(dim, aspect_ratio, width, height))
    return int(height), int(width), int(dim)


class ConveNetOps:
    """The network of conve.py:75-101 over the reference's module names (convolution, bn1, bn2, projection,
    feature_map_dropout, projection_dropout) and shape attributes (emb_height, emb_width, filter_size, padding) -- mixed
    into ConvEScorer here and into the plugin's HipConvEScorer, whose modules the reference's constructor builds."""

    def network(self, s_emb: Tensor, p_emb: Tensor) -> Tensor:
        """x [n, d] of conve.py:81-93"""
        n = p_emb.size(0)
        s2 = s_emb[:, 1:].reshape(-1, 1, int(self.emb_height), int(self.emb_width))
        p2 = p_emb[:, 1:].reshape(-1, 1, int(self.emb_height), int(self.emb_width))
        out = self.convolution(torch.cat([s2, p2], 2))
        out = torch.relu(self.bn1(out))
        out = self.feature_map_dropout(out)
        out = self.projection(out.view(n, -1))
        out = self.projection_dropout(out)
        return torch.relu(self.bn2(out))

    def kernel_net(self) -> "engine.ConveNet":
        return engine.ConveNet(int(self.emb_height), int(self.emb_width), int(self.filter_size), int(self.padding),
                               self.convolution.weight.detach(),
                               None if self.convolution.bias is None else self.convolution.bias.detach(),
                               self.bn1.running_mean, self.bn1.running_var, self.bn1.eps, self.projection.weight.detach(),
                               self.projection.bias.detach(), self.bn2.running_mean, self.bn2.running_var, self.bn2.eps)

    def score_emb(self, s_emb: Tensor, p_emb: Tensor, o_emb: Tensor, combine: str) -> Tensor:
        if combine not in ["sp_", "spo"]:
            raise Exception("Combine {} not supported in ConvE's score function".format(combine))
        n = p_emb.size(0)
        x = self.network(s_emb, p_emb)
        if x.is_cuda and x.dtype == torch.float32 and o_emb.dtype == torch.float32:
            q = torch.cat([torch.ones_like(x[:, :1]), x], 1)  # the gradient of column 0 is dropped by the cat
            out = _ScoreEmb.apply("distmult", combine, 1.0, q, torch.ones_like(q), o_emb)
        elif combine == "sp_":
            out = torch.mm(x, o_emb[:, 1:].transpose(1, 0)) + o_emb[:, 0]
        else:
            out = (x * o_emb[:, 1:]).sum(-1) + o_emb[:, 0]
        return out.view(n, -1)


class ConvEScorer(ConveNetOps, RelationalScorer):
    """kge/model/conve.py:9-101 on torch operations with autograd -- the TORCH ROUTE of ConvE: training mode (batch
    statistics, Dropout2d, Dropout), a recorded gradient, CPU parameters, a shape outside the kernel's gate.  Module names
    equal the reference's (convolution, bn1, bn2, projection): state_dicts interchange.  Embeddings have d + 1 columns,
    column 0 of an entity row is its bias.  On a GPU in float32 the contraction (and its backward) is the DistMult
    kernels' over the augmented query q' = [1 | x] (_ScoreEmb); on CPU it is plain torch."""

    name = "conve"

    def __init__(self, dim: int, aspect_ratio=2, filter_size: int = 3, padding: int = 0, feature_map_dropout: float = 0.2,
                 projection_dropout: float = 0.3, convolution_bias: bool = True, round_dim: bool = False,
                 dtype=torch.float32, device=None):
        super().__init__(1.0)
        self.emb_height, self.emb_width, self.emb_dim = conve_image_shape(dim, aspect_ratio, round_dim)
        self.filter_size, self.stride, self.padding = int(filter_size), 1, int(padding)
        self.feature_map_dropout = torch.nn.Dropout2d(feature_map_dropout)
        self.projection_dropout = torch.nn.Dropout(projection_dropout)
        self.convolution = torch.nn.Conv2d(1, 32, (self.filter_size, self.filter_size), stride=1, padding=self.padding,
                                           bias=bool(convolution_bias), device=device, dtype=dtype)
        self.bn1 = torch.nn.BatchNorm2d(32, affine=False, device=device, dtype=dtype)
        self.bn2 = torch.nn.BatchNorm1d(self.emb_dim, affine=False, device=device, dtype=dtype)
        ho = 2 * self.emb_height - self.filter_size + 2 * self.padding + 1
        wo = self.emb_width - self.filter_size + 2 * self.padding + 1
        if ho < 1 or wo < 1:
            raise ValueError("ConvE: filter_size {} does not fit the {} x {} image".format(
                filter_size, 2 * self.emb_height, self.emb_width))
        self.projection = torch.nn.Linear(32 * ho * wo, self.emb_dim, device=device, dtype=dtype)


class ConveRoutes:
    """Which way a ConvE model scores (mixed into ConvE here and into the plugin's HipConvE, which say where the tables
    and the scorer live: `_conve_parts()`).  Two routes:
      "kernel"  module in eval mode, no gradient recorded, float32 parameters on a GPU, a shape inside the gate of
                kge_conve_queries: the query network as ONE canonical arithmetic (engine.conve_queries), then the float32
                DistMult contraction of q' with the entity rows.  Rows of d + 1 floats miss the vectorised matrix-core
                path of the pair kernel (d % 8 == 0, 16-byte aligned rows), so the route keeps a copy of the entity
                table padded with zero columns to a multiple of 8 floats, and a matching zero-padded q'; zeros add
                exactly nothing to an fma chain.  The copy is cached on the table's version (the BF16Shadow pattern) and
                left out above padded_table_max_bytes (the plain rows then take the element path: the same scores inside
                the bound, slower).
      "torch"   everything else: ConvEScorer.score_emb."""
    padded_table_max_bytes = 1 << 30

    def _conve_parts(self):
        """(entity weight, relation weight, scorer, are both embedders pure lookups)"""
        raise NotImplementedError

    def _init_routes(self):
        self.routes = {"kernel": 0, "torch": 0}  # calls per route (what the tests assert)
        self.paddings = 0  # padded copies made (the cache's misses)
        self._pad_key, self._pad_table, self._pad_ones = None, None, None
        self._gate = None  # (shape, does kge_conve_queries take it): asked of the library once per shape

    def kernel_route(self) -> bool:
        ent, rel, sc, pure = self._conve_parts()
        if self.training or sc.training or not pure or not ent.is_cuda or ent.dtype != torch.float32 or rel.dtype != torch.float32:
            return False
        if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad or
                                        any(x.requires_grad for x in sc.parameters())):
            return False
        if int(getattr(sc, "stride", 1)) != 1:  # (the reference's option; the kernel is stride 1 by construction)
            return False
        shape = (int(sc.emb_height), int(sc.emb_width), int(sc.filter_size), int(sc.padding))
        if self._gate is None or self._gate[0] != shape:
            self._gate = (shape, engine.conve_gate(*shape))
        return self._gate[1]

    def padded_table(self):
        """[E, dp] zero-padded copy of the entity table, dp = d + 1 rounded up to 8; None above the byte cap"""
        ent = self._conve_parts()[0]
        dp = (ent.shape[1] + 7) // 8 * 8
        if ent.shape[0] * dp * ent.element_size() > self.padded_table_max_bytes:
            return None
        key = (ent._version, ent.data_ptr(), ent.device, tuple(ent.shape))
        if key != self._pad_key:
            t = torch.zeros((ent.shape[0], dp), dtype=ent.dtype, device=ent.device)
            t[:, :ent.shape[1]] = ent.detach()
            self._pad_table, self._pad_key = t, key
            self.paddings += 1
        return self._pad_table

    def _kernel_scores(self, s: Tensor, p: Tensor, o, combine: str) -> Tensor:
        ent, rel, sc, _ = self._conve_parts()
        n = s.numel()
        with torch.no_grad():
            table = self.padded_table()
            if table is None:
                table = ent.detach()
            dp = table.shape[1]
            q = torch.zeros((n, dp), dtype=torch.float32, device=ent.device)
            engine.conve_queries(sc.kernel_net(), ent.detach(), rel.detach(), s, p, out=q)
            if self._pad_ones is None or self._pad_ones.shape[0] < n or self._pad_ones.shape[1] != dp or \
                    self._pad_ones.device != ent.device:
                self._pad_ones = torch.ones((max(n, 64), dp), dtype=torch.float32, device=ent.device)
            if o is None:
                rows = table
            elif isinstance(o, range):  # (a contiguous chunk of the table: the plugin's _targets)
                rows = table[o.start:o.stop]
            else:
                rows = table[o.reshape(-1).long()]
            return engine.score_emb("distmult", q, self._pad_ones[:n], rows, combine)

    def conve_scores(self, s: Tensor, p: Tensor, o, combine: str) -> Tensor:
        """combine "sp_": [n, E] (o None) or [n, len(o)]; "spo": [n, 1]"""
        if self.kernel_route():
            self.routes["kernel"] += 1
            return self._kernel_scores(s, p, o, combine)
        self.routes["torch"] += 1
        return self._torch_scores(s, p, o, combine)


class ConvE(ConveRoutes, KgeModel):
    """kge/model/conve.py:104-144: embedders of d + 1 columns (the bias hack), score_sp and score_spo(direction="o")
    only -- use it under reciprocal relations, as the reference says.  The routes: ConveRoutes.  A fused training forward
    and backward of the network is not here (the follow-up)."""
    scorer_cls = ConvEScorer

    def __init__(self, num_entities: int, num_relations: int, dim: int, aspect_ratio=2, filter_size: int = 3,
                 padding: int = 0, feature_map_dropout: float = 0.2, projection_dropout: float = 0.3,
                 convolution_bias: bool = True, round_dim: bool = False, padded_table_max_bytes: int = 1 << 30, **kw):
        for opt in ("fused_dist_loss", "fused_f32_loss", "score_dtype"):
            if kw.get(opt):  # no ConvE kernel behind the fused losses, no bf16 scoring
                raise ValueError("ConvE: {} is not supported (the losses are composed from score_sp)".format(opt))
        h, w, d = conve_image_shape(dim, aspect_ratio, round_dim)
        net_args = dict(dim=d, aspect_ratio=aspect_ratio, filter_size=filter_size, padding=padding,
                        feature_map_dropout=feature_map_dropout, projection_dropout=projection_dropout,
                        convolution_bias=convolution_bias, round_dim=False)
        super().__init__(num_entities, num_relations, d + 1, scorer_args=net_args, **kw)
        self.padded_table_max_bytes = int(padded_table_max_bytes)
        self._init_routes()

    def _make_scorer(self, l_norm, dtype, device, scorer_args):
        return ConvEScorer(dtype=dtype, device=device, **scorer_args)

    def _conve_parts(self):
        return (self._entity_embedder.weight, self._relation_embedder.weight, self._scorer, self._fused())

    def _torch_scores(self, s, p, o, combine):
        se, pe = self._entity_embedder.embed(s), self._relation_embedder.embed(p)
        oe = self._entity_embedder.embed_all() if o is None else self._entity_embedder.embed(o)
        return self._scorer.score_emb(se, pe, oe, combine)

    def tables(self, flags: int = 0):
        raise ValueError("ConvE: there are no kge_tables of a ConvE model (its score is not a function of three rows)")

    def set_touched_rows(self, pair, rel_pair=None):
        if pair is not None:
            raise ValueError("ConvE: touched_rows is not supported")
        self._touched_rows = None

    def score_spo(self, s: Tensor, p: Tensor, o: Tensor, direction=None) -> Tensor:
        if direction != "o":
            raise ValueError("ConvE can only score objects")
        return self.conve_scores(s, p, o, "spo").view(-1)

    def score_sp(self, s: Tensor, p: Tensor, o: Tensor = None) -> Tensor:
        return self.conve_scores(s, p, o, "sp_")

    def score_po(self, p: Tensor, o: Tensor, s: Tensor = None) -> Tensor:
        raise Exception("Combine {} not supported in ConvE's score function".format("_po"))

    def score_sp_po(self, s: Tensor, p: Tensor, o: Tensor, entity_subset: Tensor = None) -> Tensor:
        raise Exception("Combine {} not supported in ConvE's score function".format("_po"))

    def score_so(self, s: Tensor, o: Tensor, p: Tensor = None) -> Tensor:
        raise Exception("Combine {} not supported in ConvE's score function".format("s_o"))

    def score_neg(self, s, p, o, slot, neg):
        raise ValueError("ConvE: negative-sampling blocks (score_neg) are not supported")

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        raise ValueError("ConvE: negative-sampling blocks (score_neg_shared) are not supported")

    def score_neg_blocks(self, s, p, o, neg_s=None, neg_o=None):
        raise ValueError("ConvE: negative-sampling blocks (score_neg_blocks) are not supported")


MODELS = {"complex": ComplEx, "distmult": DistMult, "transe": TransE, "rotate": RotatE, "transh": TransH,
          "rescal": Rescal, "relational_tucker3": RelationalTucker3, "conve": ConvE}


def create(model: str, num_entities: int, num_relations: int, dim: int, **kw) -> KgeModel:
    return MODELS[model](num_entities, num_relations, dim, **kw)


# ---- autograd glue (the reference gets backward from torch autograd; here the twins in
# ---- csrc/bwd.hip are called explicitly) --------------------------------------------------
def predict_filters(filter_index, direction: str, a: Tensor, p: Tensor, device):
    """The filter sets of predict_o / predict_s for `engine.topk` / `topk_composed`: [] without an index, else one
    (begin [n], end [n], col [nnz]) over the known answers of (a_i, p_i, ?) (direction "sp_": the index's (s, p) -> o
    side) or (?, p_i, a_i) ("_po": its (p, o) -> s side).  The index's arrays are put on `device` once and cached on
    the index object; on a GPU the ranges come from engine.filter_lookup (no host work per call)."""
    if filter_index is None:
        return []
    cache = filter_index.__dict__.setdefault("_predict_arrays", {})
    side = "sp" if direction == "sp_" else "po"
    arrays = cache.get((str(device), side))
    if arrays is None:
        keys, starts, values = filter_index._sp if side == "sp" else filter_index._po
        arrays = cache[(str(device), side)] = tuple(
            torch.from_numpy(x.astype("int64")).to(device) for x in (keys, starts, values))
    keys, starts, values = arrays
    a, p = a.reshape(-1).to(device), p.reshape(-1).to(device)
    first, second, mult = (a, p, filter_index.R) if side == "sp" else (p, a, filter_index.E)
    n = a.numel()
    begin = torch.zeros(n, dtype=torch.int64, device=device)
    end = torch.zeros(n, dtype=torch.int64, device=device)
    if keys.numel() and n:
        if begin.is_cuda:
            engine.filter_lookup(keys, starts, first, second, mult, begin, end)
        else:
            key = first.long() * mult + second.long()
            pos = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
            hit = keys[pos] == key
            begin = torch.where(hit, starts[pos], begin)
            end = torch.where(hit, starts[pos + 1], end)
    return [(begin, end, values)]


def topk_composed(scores: Tensor, k: int, filters=(), keep: Tensor = None, col_begin: int = 0):
    """kge_topk's result from a score matrix [n, m] (columns = the entities col_begin ..) with torch operations --
    predict_o / predict_s where the fused path does not apply (CPU tensors, dropout in training mode).  The same rule:
    canonical scores (NaN -> -inf, -0.0 -> +0.0), the filters' columns dropped except keep[i], a STABLE sort on
    (-value, id) -- never torch.topk, which leaves the order among equal scores open --, (-inf, -1) behind a row's
    last column."""
    s = scores.detach().float()
    n, m = s.shape
    neg_inf = torch.full((), float("-inf"), dtype=s.dtype, device=s.device)
    s = torch.where(torch.isnan(s), neg_inf, s)
    s = torch.where(s == 0, torch.zeros((), dtype=s.dtype, device=s.device), s)
    drop = torch.zeros((n, m), dtype=torch.bool, device=s.device)
    rows = torch.arange(n, device=s.device)
    for begin, end, col in filters:
        cnt = (end - begin).clamp_(min=0)
        total = int(cnt.sum())
        if total == 0:
            continue
        r = torch.repeat_interleave(rows, cnt)
        first = torch.cumsum(cnt, 0) - cnt
        e = torch.arange(total, device=s.device) - first[r] + begin[r]
        j = col[e] - col_begin
        ok = (j >= 0) & (j < m)
        if keep is not None:
            ok &= col[e] != keep.reshape(-1).to(s.device).long()[r]
        drop[r[ok], j[ok]] = True
    # lexicographic (dropped, -value, id): two stable sorts, the minor key first
    order = torch.sort(-s, dim=1, stable=True).indices
    order = torch.gather(order, 1, torch.sort(torch.gather(drop, 1, order).to(torch.uint8), dim=1, stable=True).indices)
    order = order[:, :k]
    live = ~torch.gather(drop, 1, order)
    val = torch.where(live, torch.gather(s, 1, order), neg_inf)
    idx = torch.where(live, order + col_begin, torch.full((), -1, dtype=torch.int64, device=s.device))
    if k > m:
        val = torch.cat((val, torch.full((n, k - m), float("-inf"), dtype=s.dtype, device=s.device)), dim=1)
        idx = torch.cat((idx, torch.full((n, k - m), -1, dtype=torch.int64, device=s.device)), dim=1)
    return val, idx


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _scatter_rows(grad_table, idx, rows):
    grad_table.index_add_(0, idx.reshape(-1).long(), rows)


def _touched_pair(t, touched):
    """`touched` = (grad, bitmap) of kge_amd.optim.Adagrad.enable_touched_rows for the entity table, checked: the
    backward then accumulates the entity gradient into the persistent `grad`, marks the rows it adds to in `bitmap`
    and returns None for the table -- no zeros_like(ent) fill, no dense gradient for the optimizer to sweep.
    Or ((grad, bitmap), (rel_grad, rel_bitmap)): the pairs of kge_amd.optim.SparseAdam.enable_touched_rows for the
    entity AND the relation table -> (entity pair, relation pair or None)."""
    ent, rel = (touched, None) if torch.is_tensor(touched[0]) else touched
    grad, bitmap = ent
    if not (grad.shape == t.ent.shape and grad.dtype == torch.float32 and t.ent.dtype == torch.float32
            and grad.device == t.ent.device and grad.stride(1) == 1):
        raise ValueError("kge_amd: the touched-row gradient buffer is a float32 tensor of the entity table's shape on "
                         "its device")
    if rel is not None:
        rgrad, _ = rel
        if not (rgrad.shape == t.rel.shape and rgrad.dtype == torch.float32 and t.rel.dtype == torch.float32
                and rgrad.device == t.rel.device and rgrad.stride(1) == 1):
            raise ValueError("kge_amd: the relation table's touched-row gradient buffer is a float32 tensor of the "
                             "table's shape on its device")
    return ent, rel


def _mark_touched(t, bitmap, *ids):
    for x in ids:
        if x is not None:
            engine.touched_mark(x, bitmap, t.ent.shape[0])


def _touched_buffers(t, touched, p, *ent_ids):
    """What a backward node on the touched-row route accumulates into -> (entity gradient buffer, relation gradient,
    whether the relation gradient is a persistent buffer too).  Marks `ent_ids` in the entity bitmap; with a relation
    pair also the batch's `p` in the relation bitmap, and the relation gradient is that pair's buffer instead of a
    fresh zeros_like(rel).  A pair that keeps a `pending` flag (kge_amd.optim.SparseAdam) is told a backward ran."""
    ent, rel = touched
    _mark_touched(t, ent[1], *ent_ids)
    if hasattr(ent, "pending"):
        ent.pending = True
    if rel is None:
        return ent[0], torch.zeros_like(t.rel), False
    engine.touched_mark(p, rel[1], t.rel.shape[0])
    if hasattr(rel, "pending"):
        rel.pending = True
    return ent[0], rel[0], True


class _ScoreSPO(torch.autograd.Function):
    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, p, o, touched=None):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        ctx.t, ctx.idx = t, (s, p, o)
        ctx.touched = None if touched is None else _touched_pair(t, touched)
        out = engine.score_spo(t, s, p, o)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        s, p, o = ctx.idx
        (scores,) = ctx.saved_tensors
        if ctx.touched is not None:  # the accumulate route on the persistent buffer, or nothing
            ge, gr, rel_kept = _touched_buffers(ctx.t, ctx.touched, p, s, o)
            if not engine.score_spo_bwd_accum(ctx.t, s, p, o, gout.contiguous(), scores, ge, gr):
                raise RuntimeError("kge_amd: kge_score_spo_bwd_accum declined a shape the touched-row step admitted")
            return None, None, None, None if rel_kept else gr, None, None, None, None
        ge, gr = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel)
        # one kernel: row gradients accumulated into the table gradients (runs of equal s / p
        # summed in registers first); fallback: row gradients + three scatter-adds
        if not engine.score_spo_bwd_accum(ctx.t, s, p, o, gout.contiguous(), scores, ge, gr):
            g_s, g_p, g_o = engine.score_spo_bwd(ctx.t, s, p, o, gout.contiguous(), scores)
            _scatter_rows(ge, s, g_s)
            _scatter_rows(ge, o, g_o)
            _scatter_rows(gr, p, g_p)
        return None, None, ge, gr, None, None, None, None


class _ScoreNeg(torch.autograd.Function):
    """[n, K] scores of the positives with `slot` (0 = s, 2 = o) replaced by neg[i, k] -- what
    BatchNegativeSample.score computes with implementation "triple" (sampler.py:291-306) -- from
    kge_score_neg; backward = kge_score_neg_bwd_accum (complete table gradients, no [n*K, 3] index
    tensor and no [n*K, d] gathered rows in either pass)."""

    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, p, o, slot, neg, touched=None):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        out = engine.score_neg(t, s, p, o, slot, neg)
        ctx.t, ctx.idx, ctx.slot = t, (s, p, o, neg), slot
        ctx.touched = None if touched is None else _touched_pair(t, touched)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        s, p, o, neg = ctx.idx
        (scores,) = ctx.saved_tensors
        if ctx.touched is not None:  # the accumulate kernel on the persistent buffer, or nothing
            ge, gr, rel_kept = _touched_buffers(ctx.t, ctx.touched, p, s, o, neg)
            if not engine.score_neg_bwd_accum(ctx.t, s, p, o, ctx.slot, neg, gout, scores, ge, gr):
                raise RuntimeError("kge_amd: kge_score_neg_bwd_accum declined a shape the touched-row step admitted")
            return None, None, None, None if rel_kept else gr, None, None, None, None, None, None
        ge, gr = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel)
        if not engine.score_neg_bwd_accum(ctx.t, s, p, o, ctx.slot, neg, gout, scores, ge, gr):
            # shapes the accumulate kernel does not take (bf16 parameters, d > 1024): expanded triples
            K = neg.shape[1]
            tr = [x.reshape(-1).long().repeat_interleave(K) for x in (s, p, o)]
            tr[ctx.slot] = neg.reshape(-1).long()
            g_s, g_p, g_o = engine.score_spo_bwd(ctx.t, tr[0], tr[1], tr[2], gout.reshape(-1).contiguous(),
                                                 scores.reshape(-1))
            ge, gr = ge.float(), gr.float()
            _scatter_rows(ge, tr[0], g_s)
            _scatter_rows(ge, tr[2], g_o)
            _scatter_rows(gr, tr[1], g_p)
            ge, gr = ge.to(ctx.t.ent.dtype), gr.to(ctx.t.rel.dtype)
        return None, None, ge, gr, None, None, None, None, None, None


# ---- embedder dropout inside the triple-wise kernels (include/kge_amd.h "Embedder dropout") ----------------
DROPOUT_TRIPLE_SCORERS = ("complex", "distmult", "transe", "rotate")
DROPOUT_CALLS = 0  # fused dropout calls of this process (the plugin's tests count them)


def dropout_triple_fusable(name: str, ent: Tensor, rel: Tensor, p_ent: float, p_rel: float) -> bool:
    """What kge_score_spo_dropout / kge_score_neg_dropout and their backward take: float32 GPU tables of the four
    scorers, dim <= 1024, probabilities in [0, 1) that are not both 0."""
    return (name in DROPOUT_TRIPLE_SCORERS and ent.is_cuda and rel.is_cuda and ent.dtype == torch.float32 and
            rel.dtype == torch.float32 and ent.shape[1] <= 1024 and 0.0 <= p_ent < 1.0 and 0.0 <= p_rel < 1.0 and
            (p_ent > 0.0 or p_rel > 0.0))


class DropoutClock:
    """The (seed, call) source of a model's fused dropout calls: `seed` taken from torch.initial_seed() where the model
    is built (settable), `call` a host counter incremented once per fused dropout call."""

    def __init__(self, seed=None):
        self.seed = int(torch.initial_seed() if seed is None else seed)
        self.call = 0

    def next(self, p_ent: float, p_rel: float) -> engine.Dropout:
        global DROPOUT_CALLS
        self.call += 1
        DROPOUT_CALLS += 1
        return engine.Dropout(float(p_ent), float(p_rel), self.seed, self.call)


class _ScoreSPODropout(torch.autograd.Function):
    """_ScoreSPO with the embedder dropout of the three gathered rows inside the kernels: the forward's Dropout record
    (seed, call) is saved and handed to the backward, which regenerates the masks."""

    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, p, o, dropout, touched=None):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        ctx.t, ctx.idx, ctx.dropout = t, (s, p, o), dropout
        ctx.touched = None if touched is None else _touched_pair(t, touched)
        out = engine.score_spo_dropout(t, s, p, o, dropout)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        s, p, o = ctx.idx
        (scores,) = ctx.saved_tensors
        if ctx.touched is not None:
            ge, gr, rel_kept = _touched_buffers(ctx.t, ctx.touched, p, s, o)
        else:
            ge, gr, rel_kept = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel), False
        if not engine.score_spo_dropout_bwd_accum(ctx.t, s, p, o, gout.contiguous(), scores, ge, gr, ctx.dropout):
            raise RuntimeError("kge_amd: kge_score_spo_dropout_bwd_accum declined a shape its forward took")
        if ctx.touched is not None:
            return None, None, None, None if rel_kept else gr, None, None, None, None, None
        return None, None, ge, gr, None, None, None, None, None


class _ScoreNegDropout(torch.autograd.Function):
    """_ScoreNeg with the embedder dropout inside the kernels: the fixed rows of a positive masked once, every corrupted
    row occurrence with its own mask; the backward regenerates them from the forward's Dropout record."""

    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, p, o, slot, neg, dropout, touched=None):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        out = engine.score_neg_dropout(t, s, p, o, slot, neg, dropout)
        ctx.t, ctx.idx, ctx.slot, ctx.dropout = t, (s, p, o, neg), slot, dropout
        ctx.touched = None if touched is None else _touched_pair(t, touched)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        s, p, o, neg = ctx.idx
        (scores,) = ctx.saved_tensors
        if ctx.touched is not None:
            ge, gr, rel_kept = _touched_buffers(ctx.t, ctx.touched, p, s, o, neg)
        else:
            ge, gr, rel_kept = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel), False
        if not engine.score_neg_dropout_bwd_accum(ctx.t, s, p, o, ctx.slot, neg, gout, scores, ge, gr, ctx.dropout):
            raise RuntimeError("kge_amd: kge_score_neg_dropout_bwd_accum declined a shape its forward took")
        if ctx.touched is not None:
            return None, None, None, None if rel_kept else gr, None, None, None, None, None, None, None
        return None, None, ge, gr, None, None, None, None, None, None, None


class _ScoreNegShared(torch.autograd.Function):
    """[n, K] scores of the positives against a SHARED negative sample (unique ids, drop indexes or None, repeat
    columns): what NaiveSharedNegativeSample.score / DefaultSharedNegativeSample.score return (sampler.py:428-463,
    537-578), from kge_score_neg_shared -- the target rows staged once per workgroup, no [n, K] sample tensor and no
    [n, Uc + 1] intermediate score matrix; backward = kge_score_neg_shared_bwd_accum (complete table gradients, one
    row flush per (positive, tile) and (unique row, tile) instead of one atomic per occurrence)."""

    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, p, o, slot, unique, drop, repeat):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        out = engine.score_neg_shared(t, s, p, o, slot, unique, drop, repeat)
        ctx.t, ctx.idx, ctx.slot = t, (s, p, o, unique, drop, repeat), slot
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        s, p, o, unique, drop, repeat = ctx.idx
        (scores,) = ctx.saved_tensors
        ge, gr = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel)
        if not engine.score_neg_shared_bwd_accum(ctx.t, s, p, o, ctx.slot, unique, drop, repeat, gout, scores, ge, gr):
            # shapes the shared accumulate kernel does not take: the per-triple route on the materialised samples
            neg = engine.shared_samples(unique, drop, repeat, scores.shape[0]).contiguous()
            if not engine.score_neg_bwd_accum(ctx.t, s, p, o, ctx.slot, neg, gout, scores, ge, gr):
                K = neg.shape[1]
                tr = [x.reshape(-1).long().repeat_interleave(K) for x in (s, p, o)]
                tr[ctx.slot] = neg.reshape(-1).long()
                g_s, g_p, g_o = engine.score_spo_bwd(ctx.t, tr[0], tr[1], tr[2], gout.reshape(-1).contiguous(),
                                                     scores.reshape(-1))
                ge, gr = ge.float(), gr.float()
                _scatter_rows(ge, tr[0], g_s)
                _scatter_rows(ge, tr[2], g_o)
                _scatter_rows(gr, tr[1], g_p)
                ge, gr = ge.to(ctx.t.ent.dtype), gr.to(ctx.t.rel.dtype)
        return None, None, ge, gr, None, None, None, None, None, None, None


class _ScoreSO(torch.autograd.Function):
    """[n, m] scores of (s[i], rels[j], o[i]) -- rels None: all relations -- = KgeModel.score_so (kge_model.py:727-747)
    from kge_score_so: the relation rows staged once per workgroup, none of the three [n m, d] repeats of the
    reference's composition (kge_model.py:202-209) in either pass; backward = kge_score_so_bwd_accum (complete table
    gradients, one row flush per (pair, tile) and (relation, tile))."""

    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, o, rels, touched=None):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        out = engine.score_so(t, s, o, rels)
        ctx.t, ctx.idx = t, (s, o, rels)
        ctx.touched = None if touched is None else _touched_pair(t, touched)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        s, o, rels = ctx.idx
        (scores,) = ctx.saved_tensors
        if ctx.touched is not None:  # the accumulate kernel on the persistent buffers, or nothing
            p = rels if rels is not None else torch.arange(ctx.t.rel.shape[0], device=ctx.t.rel.device)
            ge, gr, rel_kept = _touched_buffers(ctx.t, ctx.touched, p, s, o)
            if not engine.score_so_bwd(ctx.t, s, o, rels, gout, scores, ge, gr):
                raise RuntimeError("kge_amd: kge_score_so_bwd_accum declined a shape the touched-row step admitted")
            return None, None, None, None if rel_kept else gr, None, None, None, None
        ge, gr = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel)
        if not engine.score_so_bwd(ctx.t, s, o, rels, gout, scores, ge, gr):
            raise RuntimeError("kge_amd: kge_score_so_bwd_accum declined tables score_so admitted")
        return None, None, ge, gr, None, None, None, None


def score_so_fusable(name: str, ent: torch.Tensor, rel: torch.Tensor, n: int) -> bool:
    """Where KgeModel.score_so runs kge_score_so: one of its four scorers, tables on a GPU that the kernel takes, and
    -- with a recorded gradient -- tables kge_score_so_bwd_accum takes (float32, dim <= 1024); anything else goes the
    composed way (bf16 tables under autograd included, as score_neg does where its backward declines)."""
    if not ent.is_cuda or not engine.score_so_supported(name, ent.dtype, ent.shape[1], n):
        return False
    if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad):
        return ent.dtype == torch.float32 and rel.dtype == torch.float32 and ent.shape[1] <= 1024
    return True


class _ScoreNegBlocks(torch.autograd.Function):
    """What TrainingJobNegativeSampling._process_subbatch scores for a subbatch (train_negative_sampling.py:120-151) in
    ONE autograd node: the positives (score_spo) and the negative blocks of the subject and the object slot
    (BatchNegativeSample.score, sampler.py:263-306).  Its backward accumulates all three into ONE pair of dense table
    gradients (kge_score_spo_bwd_accum + kge_score_neg_bwd_accum per slot on the same buffers) -- composed from
    _ScoreSPO / _ScoreNeg every node brings its own zero-filled [E, d] gradient and autograd adds them up: six fills and
    six adds of the entity table's size per step (0.2 of a 1.6 ms step at the WN18RR shape).  float32 tables, dim <= 1024
    (the accumulate kernels' domain; the caller checks)."""

    @staticmethod
    def forward(ctx, name, l_norm, ent, rel, s, p, o, neg_s, neg_o, touched=None):
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        pos = engine.score_spo(t, s, p, o)
        sc_s = engine.score_neg(t, s, p, o, 0, neg_s) if neg_s is not None else None
        sc_o = engine.score_neg(t, s, p, o, 2, neg_o) if neg_o is not None else None
        ctx.t, ctx.idx = t, (s, p, o, neg_s, neg_o)
        ctx.touched = None if touched is None else _touched_pair(t, touched)
        ctx.save_for_backward(pos, sc_s, sc_o)
        return pos, sc_s, sc_o

    @staticmethod
    def backward(ctx, g_pos, g_s, g_o):
        s, p, o, neg_s, neg_o = ctx.idx
        pos, sc_s, sc_o = ctx.saved_tensors
        rel_kept = False
        if ctx.touched is not None:
            # the persistent buffer in place of a fresh zeros_like(ent); s, o and the blocks differentiated are marked
            ge, gr, rel_kept = _touched_buffers(ctx.t, ctx.touched, p, s, o, neg_s if g_s is not None else None,
                                                neg_o if g_o is not None else None)
        else:
            ge, gr = torch.zeros_like(ctx.t.ent), torch.zeros_like(ctx.t.rel)
        if g_pos is not None and not engine.score_spo_bwd_accum(ctx.t, s, p, o, g_pos.contiguous(), pos, ge, gr):
            raise RuntimeError("kge_amd: kge_score_spo_bwd_accum declined a shape score_neg_blocks admitted")
        for slot, neg, g, sc in ((0, neg_s, g_s, sc_s), (2, neg_o, g_o, sc_o)):
            if neg is not None and g is not None:
                if not engine.score_neg_bwd_accum(ctx.t, s, p, o, slot, neg, g, sc, ge, gr):
                    raise RuntimeError("kge_amd: kge_score_neg_bwd_accum declined a shape score_neg_blocks admitted")
        return (None, None, None if ctx.touched is not None else ge, None if rel_kept else gr, None, None, None, None,
                None, None)


def neg_shared_fusable(ent: torch.Tensor, n: int) -> bool:
    """The shapes kge_score_neg_shared takes (a row that fits its LDS tile, a grid that fits): anything else goes the
    per-triple way on engine.shared_samples -- or, in the plugin, back to the sampler's own score."""
    return engine.neg_shared_supported(ent.dtype, ent.shape[1], n)


def neg_blocks_fusable(ent: torch.Tensor, rel: torch.Tensor) -> bool:
    return (ent.is_cuda and ent.dtype == torch.float32 and rel.dtype == torch.float32 and ent.shape[1] <= 1024
            and ent.is_contiguous() and rel.is_contiguous())


def _bf16_copy_of(param):
    from .optim import bf16_copy_of  # (copy, version, data_ptr of the master) must all still match
    return bf16_copy_of(param)


class BF16Shadow:
    """bf16 copies of f32 master tables for mixed-precision scoring (`score_dtype: bfloat16`):
    the forward runs the bf16 matrix-core kernel on the copies, the backward differentiates the
    f32 masters.  With autograd enabled (training) the copies are re-cast on every call (two
    15 MB writes at the FB15k-237 shape, ~10 us); without (evaluation) only when a master's
    storage or version counter changed -- in-place edits through `.data` do not bump the
    counter, hence no caching while training."""

    def __init__(self):
        self._key, self._tables = None, None

    def tables(self, name, ent, rel, l_norm) -> "engine.Tables":
        # copies written by the optimizer's own pass over the tables (kge_amd.optim.Adagrad with
        # bf16_copies=True) are fresh by construction: no cast at all
        e16, r16 = _bf16_copy_of(ent), _bf16_copy_of(rel)
        if e16 is not None and r16 is not None:
            key = (e16.data_ptr(), ent._version, ent.data_ptr(), r16.data_ptr(), rel._version, rel.data_ptr(), "opt")
            if key != self._key:
                self._tables, self._key = engine.Tables(name, e16, r16, l_norm), key
            return self._tables
        key = (ent.data_ptr(), ent._version, rel.data_ptr(), rel._version)
        if key != self._key or torch.is_grad_enabled():
            self._tables = engine.Tables(name, ent.detach().to(torch.bfloat16), rel.detach().to(torch.bfloat16),
                                         l_norm)
            self._key = key
        return self._tables


class _ScorePairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, name, l_norm, direction, ent, rel, a, p, targets, fwd_tables=None, padded=False, rel_rows=False):
        # rel_rows: `rel` holds one row per query and p is arange(n) (RelationalTucker3's "batch" route) -- the per-row
        # relation gradient of the backward IS the gradient of `rel`
        ctx.rel_rows = bool(rel_rows)
        t = engine.Tables(name, ent.detach(), rel.detach(), l_norm)
        tf = t if fwd_tables is None else fwd_tables  # mixed precision: bf16 copies, forward only
        # padded (the models' `padded_scores` option, honoured where no gradient is recorded): the scores as the [:, :m]
        # view of a matrix with sector-aligned rows (engine.score_pitch)
        out = (engine.score_sp if direction == "sp" else engine.score_po)(tf, *((a, p) if direction == "sp" else (p, a)), targets,
                                                                          padded=bool(padded))
        ctx.t, ctx.direction, ctx.idx = t, direction, (a, p, targets)
        ctx.tf = fwd_tables
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, p, targets = ctx.idx
        (scores,) = ctx.saved_tensors
        # mixed precision: both gradient products on the bf16 matrix cores too (bf16 copies of the
        # tables, gout rounded to bf16, f32 accumulation) -- autocast semantics
        g_a, g_p, g_t = engine.score_pairs_bwd(ctx.tf if ctx.tf is not None else ctx.t, ctx.direction, a, p,
                                               targets, gout, scores)
        if ctx.rel_rows:
            if g_p.shape != ctx.t.rel.shape:
                raise RuntimeError("kge_amd: rel_rows needs one relation row per query")
            gr = g_p  # (no d^2-wide zero fill and index_add_)
        else:
            gr = torch.zeros_like(ctx.t.rel)
            _scatter_rows(gr, p, g_p)
        if targets is None:
            ge = g_t  # [E, d], fresh: the dense target gradient IS the table gradient, plus the query rows
        else:
            ge = torch.zeros_like(ctx.t.ent)
            _scatter_rows(ge, targets, g_t)
        _scatter_rows(ge, a, g_a)
        return None, None, None, ge, gr, None, None, None, None, None, None


class _LossRows(torch.autograd.Function):
    """What the nine one-sided loss nodes below share: per-row loss fused with the sp_ / _po scoring against all entities
    -- 1vsAll cross entropy, KvsAll KL, KvsAll BCE (labels as an int64 CSR: rowptr [n + 1], col [nnz], ids in any order)
    -- on one of three kinds of tables (bf16: `tables16`, the parameters or their bf16 copies in mixed precision;
    TransE / RotatE on float32; ComplEx / DistMult on float32: `tables`, the parameters themselves, the backward walking
    the entity columns in chunks of `chunk_cols`, 0 = the library's default).  Gradients go to `ent` / `rel`.  A node's
    forward names its inputs (its `apply` signature) and hands them to `rows` with its pair of engine functions."""

    @staticmethod
    def rows(ctx, fwd, bwd, tables, direction, rel, idx, tail=(), **bwd_kw):
        """The loss rows of fwd(tables, direction, *idx, *tail), which returns them alone or with the rows' lse; the
        backward calls bwd(tables, direction, *idx, [lse,] g_rows=.., **bwd_kw).  idx[0] / idx[1]: the query rows' entity
        and relation ids."""
        out = fwd(tables, direction, *idx, *tail)
        ctx.call, ctx.rel_shape = (bwd, tables, direction, idx, bwd_kw), rel.shape
        if isinstance(out, tuple):
            out, lse = out
            ctx.save_for_backward(lse)
        return out

    @staticmethod
    def backward(ctx, g_rows):
        bwd, tables, direction, idx, bwd_kw = ctx.call
        g_a, g_p, ge = bwd(tables, direction, *idx, *ctx.saved_tensors, g_rows=g_rows.contiguous(), **bwd_kw)
        gr = torch.zeros(ctx.rel_shape, dtype=torch.float32, device=ge.device)
        _scatter_rows(gr, idx[1], g_p)
        _scatter_rows(ge, idx[0], g_a)  # ge [E, d] is fresh: the dense target gradient + the query rows
        return (None, ge, gr) + (None,) * (len(ctx.needs_input_grad) - 3)  # (direction, ent, rel, the other inputs)


class _FusedCE(_LossRows):
    """1vsAll cross entropy on bf16 tables (kge_ce_fwd / kge_ce_bwd)."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, label, tables16):
        return _LossRows.rows(ctx, engine.ce_fwd, engine.ce_bwd, tables16, direction, rel, (a, p, label))


class _FusedCEDist(_LossRows):
    """_FusedCE for TransE / RotatE on float32 tables (kge_ce_dist_fwd / kge_ce_dist_bwd)."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, label, tables, chunk_cols=0):
        return _LossRows.rows(ctx, engine.ce_dist_fwd, engine.ce_dist_bwd, tables, direction, rel, (a, p, label),
                              (chunk_cols,), chunk_cols=chunk_cols)


class _FusedCEF32(_LossRows):
    """_FusedCE for ComplEx / DistMult on FLOAT32 tables (kge_ce_f32_fwd / kge_ce_f32_bwd)."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, label, tables, chunk_cols=0):
        return _LossRows.rows(ctx, engine.ce_f32_fwd, engine.ce_f32_bwd, tables, direction, rel, (a, p, label),
                              (chunk_cols,), chunk_cols=chunk_cols)


class _FusedKL(_LossRows):
    """KvsAll KL loss on bf16 tables (kge_kl_fwd / kge_kl_bwd).  label_weight / label_bias [n] or None: the two terms of
    smoothed labels (kl_fused composes label smoothing around this node or _FusedKLF32; label_bias, the uniform term,
    is taken inside the gradient kernel -- these scores are linear in the target row)."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, rowptr, col, label_weight, label_bias, tables16):
        return _LossRows.rows(ctx, engine.kl_fwd, engine.kl_bwd, tables16, direction, rel, (a, p, rowptr, col),
                              (label_weight,), label_weight=label_weight, label_bias=label_bias)


class _FusedKLDist(_LossRows):
    """_FusedKL for TransE / RotatE on float32 tables (kge_kl_dist_fwd / kge_kl_dist_bwd); no label-smoothing bias."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, rowptr, col, label_weight, tables, chunk_cols=0):
        return _LossRows.rows(ctx, engine.kl_dist_fwd, engine.kl_dist_bwd, tables, direction, rel, (a, p, rowptr, col),
                              (label_weight, chunk_cols), label_weight=label_weight, chunk_cols=chunk_cols)


class _FusedKLF32(_LossRows):
    """_FusedKL for ComplEx / DistMult on FLOAT32 tables (kge_kl_f32_fwd / kge_kl_f32_bwd); _FusedKL's signature."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, rowptr, col, label_weight, label_bias, tables, chunk_cols=0):
        return _LossRows.rows(ctx, engine.kl_f32_fwd, engine.kl_f32_bwd, tables, direction, rel, (a, p, rowptr, col),
                              (label_weight, chunk_cols), label_weight=label_weight, label_bias=label_bias,
                              chunk_cols=chunk_cols)


class _FusedBCE(_LossRows):
    """KvsAll BCE-with-logits, summed over all entities, on bf16 tables (kge_bce_fwd / kge_bce_bwd); bce_fused composes
    label smoothing around this node or _FusedBCEF32."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, rowptr, col, offset, tables16):
        return _LossRows.rows(ctx, engine.bce_fwd, engine.bce_bwd, tables16, direction, rel, (a, p, rowptr, col, offset))


class _FusedBCEDist(_LossRows):
    """_FusedBCE for TransE / RotatE on float32 tables (kge_bce_dist_fwd / kge_bce_dist_bwd)."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, rowptr, col, offset, tables, chunk_cols=0):
        return _LossRows.rows(ctx, engine.bce_dist_fwd, engine.bce_dist_bwd, tables, direction, rel,
                              (a, p, rowptr, col, offset), (chunk_cols,), chunk_cols=chunk_cols)


class _FusedBCEF32(_LossRows):
    """_FusedBCE for ComplEx / DistMult on FLOAT32 tables (kge_bce_f32_fwd / kge_bce_f32_bwd); _FusedBCE's signature."""

    @staticmethod
    def forward(ctx, direction, ent, rel, a, p, rowptr, col, offset, tables, chunk_cols=0):
        return _LossRows.rows(ctx, engine.bce_f32_fwd, engine.bce_f32_bwd, tables, direction, rel,
                              (a, p, rowptr, col, offset), (chunk_cols,), chunk_cols=chunk_cols)


class _FusedCE2(torch.autograd.Function):
    """Both directions of a 1vsAll batch (kge_ce_sp_po_fwd / _bwd): [2n] loss rows, sp_ queries
    first; one scoring launch and one pair of gradient products for the whole batch."""

    @staticmethod
    def forward(ctx, ent, rel, s, p, o, tables16):
        loss_rows, lse = engine.ce_sp_po_fwd(tables16, s, p, o)
        ctx.t16, ctx.idx, ctx.rel_shape = tables16, (s, p, o), rel.shape
        ctx.save_for_backward(lse)
        return loss_rows

    @staticmethod
    def backward(ctx, g_rows):
        s, p, o = ctx.idx
        (lse,) = ctx.saved_tensors
        # complete table gradients from the library (the scatter-add of the gathered rows included)
        ge, gr = engine.ce_sp_po_bwd_accum(ctx.t16, s, p, o, lse, g_rows=g_rows.contiguous())
        return ge, gr, None, None, None, None


class _FusedCE2Sum(torch.autograd.Function):
    """scale * sum of _FusedCE2's rows as a 0-d tensor (kge_ce_sp_po_fwd_sum / kge_ce_sp_po_bwd_accum_sum): the sum
    leaves the combine launch, the backward reads the upstream gradient and the scale from device memory.  `scale`
    is a constant of the graph (no gradient flows into it)."""

    @staticmethod
    def forward(ctx, ent, rel, s, p, o, tables16, scale):
        # keep_queries: the forward's build launch also leaves the gradient products' query matrix in the workspace, and
        # the backward -- if it is the NEXT call on that workspace (the generation count says so: a training step's
        # loss.backward() right behind the loss; always true inside a captured step) -- starts from the forward's query
        # fragments instead of building them again: one launch less per step
        total, _rows, lse = engine.ce_sp_po_fwd_sum(tables16, s, p, o, scale, keep_queries=True)
        ctx.t16, ctx.idx, ctx.scale = tables16, (s, p, o), scale
        ctx.generation = engine.ce2_generation(tables16.device)
        ctx.versions = tuple(x._version for x in (s, p, o) if torch.is_tensor(x))
        ctx.save_for_backward(lse)
        return total

    @staticmethod
    def backward(ctx, gout):
        s, p, o = ctx.idx
        (lse,) = ctx.saved_tensors
        g = gout if gout.dtype == torch.float32 and gout.is_contiguous() else gout.float().contiguous()
        kept = (engine.ce2_generation(ctx.t16.device) == ctx.generation
                and ctx.versions == tuple(x._version for x in (s, p, o) if torch.is_tensor(x)))
        ge, gr = engine.ce_sp_po_bwd_accum_sum(ctx.t16, s, p, o, lse, g=g, scale=ctx.scale, keep_queries=kept)
        return ge, gr, None, None, None, None, None


# ---- embedder dropout inside the fused 1vsAll loss ------------------------------------------------------------------
# LookupEmbedder._postprocess (kge/model/embedder/lookup_embedder.py:64-69, 102-105) applies torch.nn.Dropout to the
# rows it returns: independently to the gathered query rows (embed), to the gathered relation rows and to ALL entity
# rows (embed_all) -- score_sp(s, p) of a model in training mode scores dropout(E[s]) (x) dropout(R[p]) against
# dropout(E).  Every tuned LibKGE config sets entity / relation dropout, so a fused loss that declines it trains those
# configs on the unfused path.  Here the three masks are applied BEFORE the fused kernels -- on the float32 rows and
# on a masked copy of the table (one elementwise pass over [E, d]: ~15 MB against the [n, E] score matrix the fused loss
# does not write) --, the kernels take the dense rows (kge_ce_emb_fwd / _bwd) and torch's autograd carries the kernel's
# gradients back through the masks and the gathers.  The masks are torch's (Philox on the device) unless handed in.
def embedder_dropout(x: Tensor, p: float, mask: Tensor = None) -> Tensor:
    """torch.nn.functional.dropout(x, p, training=True) with the mask optionally given: mask (same shape, 0 / 1) keeps
    the elements where it is 1 and scales them by 1 / (1 - p)."""
    if p <= 0.0:
        return x
    if mask is None:
        return torch.nn.functional.dropout(x, p, True)
    return x * (mask.to(x.dtype) * (1.0 / (1.0 - p)))


class _FusedCEEmb(torch.autograd.Function):
    """Per-row 1vsAll cross entropy of dense query rows against all rows of a dense table (kge_ce_emb_fwd / _bwd): the
    inputs are the float32 (dropped-out) rows; they are rounded to bf16 for the matrix-core kernels inside, gradients
    come back in float32 w.r.t. the inputs."""

    @staticmethod
    def forward(ctx, scorer, l_norm, direction, table, a_rows, p_rows, label):
        t16 = engine.Tables(scorer, table.detach().to(torch.bfloat16), p_rows.detach().to(torch.bfloat16), l_norm)
        a16 = a_rows.detach().to(torch.bfloat16).contiguous()
        loss_rows, lse = engine.ce_emb_fwd(t16, direction, a16, t16.rel, label)
        ctx.t16, ctx.direction, ctx.label = t16, direction, label
        ctx.save_for_backward(a16, lse)
        return loss_rows

    @staticmethod
    def backward(ctx, g_rows):
        a16, lse = ctx.saved_tensors
        g_a, g_p, g_t = engine.ce_emb_bwd(ctx.t16, ctx.direction, a16, ctx.t16.rel, ctx.label, lse,
                                          g_rows=g_rows.contiguous())
        return None, None, None, g_t, g_a, g_p, None


def ce_fused_dropout(scorer: str, l_norm: float, direction: str, ent: Tensor, rel: Tensor, a: Tensor, p: Tensor,
                     label: Tensor, p_ent: float, p_rel: float, masks: dict = None) -> Tensor:
    """[n] cross entropy of score_sp(a, p) ("sp") / score_po(p, a) ("po") over all entities with the embedders'
    dropout applied as the reference applies it (three independent masks: "a" [n, d], "p" [n, d_r], "all" [E, d];
    `masks` may hand any of them in).  Differentiable w.r.t. the float32 tables `ent` / `rel`."""
    masks = masks or {}
    a_rows = embedder_dropout(ent[a.reshape(-1).long()], p_ent, masks.get("a"))
    p_rows = embedder_dropout(rel[p.reshape(-1).long()], p_rel, masks.get("p"))
    table = embedder_dropout(ent, p_ent, masks.get("all"))
    return _FusedCEEmb.apply(scorer, l_norm, direction, table, a_rows, p_rows, label)


class _FusedMultiLabel2(torch.autograd.Function):
    """Both query types of a KvsAll batch: (loss rows of the sp_ queries, loss rows of the _po queries), each from its
    fused forward (kge_kl_fwd / kge_bce_fwd), and ONE backward for both (kge_multilabel2_bwd_accum): two d loss / d score
    passes into one gradient matrix, the two gradient products once over all rows, the gathered rows' gradients
    scattered by the library -- where two _FusedKL nodes run four products and leave two index_add passes and a
    gradient accumulation over [E, d] to autograd (train_KvsAll.py:274-294 back-propagates the two losses separately:
    the same gradients, accumulated).  No label smoothing (its extra terms are torch ops around the per-type nodes)."""

    @staticmethod
    def forward(ctx, kind, offset, ent, rel, s, p_sp, rowptr_sp, col_sp, o, p_po, rowptr_po, col_po, tables16,
                sum_scale=None):
        # sum_scale (a float): ONE output, sum_scale * (sum of all loss rows) -- the batch loss of the training job; its
        # backward hands the upstream gradient to the kernels as a device scalar (no expand / copy / scale launches)
        lse = (None, None)
        if kind == "kl":
            rows_sp, lse_sp = engine.kl_fwd(tables16, "sp", s, p_sp, rowptr_sp, col_sp, None)
            rows_po, lse_po = engine.kl_fwd(tables16, "po", o, p_po, rowptr_po, col_po, None)
            lse = (lse_sp, lse_po)
        else:
            rows_sp = engine.bce_fwd(tables16, "sp", s, p_sp, rowptr_sp, col_sp, offset)
            rows_po = engine.bce_fwd(tables16, "po", o, p_po, rowptr_po, col_po, offset)
        ctx.t16, ctx.kind, ctx.offset, ctx.lse, ctx.sum_scale = tables16, kind, offset, lse, sum_scale
        ctx.idx = ((s, p_sp, rowptr_sp, col_sp), (o, p_po, rowptr_po, col_po))
        if sum_scale is not None:
            return (rows_sp.sum() + rows_po.sum()) * float(sum_scale)
        return rows_sp, rows_po

    @staticmethod
    def backward(ctx, *gout):
        sp, po = ctx.idx
        if ctx.sum_scale is not None:
            g = gout[0] if gout[0].dtype == torch.float32 and gout[0].is_contiguous() else gout[0].float().contiguous()
            ge, gr = engine.multilabel2_bwd_accum(ctx.t16, ctx.kind, ctx.offset, sp + (ctx.lse[0], None),
                                                  po + (ctx.lse[1], None), g=g, scale=float(ctx.sum_scale))
        else:
            ge, gr = engine.multilabel2_bwd_accum(ctx.t16, ctx.kind, ctx.offset, sp + (ctx.lse[0], gout[0].contiguous()),
                                                  po + (ctx.lse[1], gout[1].contiguous()))
        return (None, None, ge, gr) + (None,) * 10


def kl_fused(name: str, l_norm, direction: str, ent: Tensor, rel: Tensor, a: Tensor, p: Tensor, rowptr: Tensor,
             col: Tensor, eps: float, t, fused_fn=None) -> Tensor:
    """The fused KvsAll KL loss with label smoothing `eps` (train_KvsAll.py:260-266: labels =
    (1 - eps) * multi_hot + 1/E before loss.py:208-213 normalises them).  The smoothed label row is a_i on
    row i's k_i labels and b_i elsewhere (Z_i = (1 - eps) k_i + 1, a_i = (1 - eps + 1/E) / Z_i,
    b_i = (1/E) / Z_i), so
        KL_i = lse_i - (a_i - b_i) * sum_{labels} score_ij       <- kge_kl_weighted_fwd, fused
               - b_i * sum_j score_ij                            <- linear in the entity table (ComplEx and
                                                                    DistMult, the fused path's scorers): ONE
                                                                    [n, 1] score against the table's column sum
               + k_i a_i log a_i + (E - k_i) b_i log b_i         <- constant.
    fused_fn: the autograd function of the fused part, _FusedKL (bf16 tables; the default) or _FusedKLF32 (float32
    tables: `t` are then the parameters themselves)."""
    fused_fn = fused_fn or _FusedKL
    if eps == 0.0:
        return fused_fn.apply(direction, ent, rel, a, p, rowptr, col, None, None, t)
    E = ent.shape[0]
    k = (rowptr[1:] - rowptr[:-1]).to(device=ent.device, dtype=torch.float32)
    Z = (1.0 - eps) * k + 1.0
    a_w, b_w = (1.0 - eps + 1.0 / E) / Z, (1.0 / E) / Z
    # the GRADIENT of the uniform term is taken inside the gradient kernel (label_bias = b_i: b_i is subtracted at
    # every column next to the softmax), so only its VALUE is computed here
    fused = fused_fn.apply(direction, ent, rel, a, p, rowptr, col, (a_w - b_w).contiguous(), b_w.contiguous(), t)
    with torch.no_grad():
        s_all = _sum_of_scores_value(name, direction, ent, rel, a, p)
    const = k * a_w * torch.log(a_w) + (E - k) * b_w * torch.log(b_w)
    return fused - b_w * s_all + const


def _score_against_column_sum(name: str, l_norm, direction: str, ent: Tensor, rel: Tensor, a: Tensor,
                              p: Tensor) -> Tensor:
    """[n]: sum_j score(i, j) over ALL entities j.  ComplEx and DistMult are linear in the target row, so
    this is one score of each query against the entity table's column sum."""
    colsum = ent.float().sum(dim=0, keepdim=True)
    rows, prow = ent[a.long()].float(), rel[p.long()].float()
    if direction == "sp":
        return _ScoreEmb.apply(name, "sp_", l_norm, rows, prow, colsum).view(-1)
    return _ScoreEmb.apply(name, "_po", l_norm, colsum, prow, rows).view(-1)


def _sum_of_scores_value(name: str, direction: str, ent: Tensor, rel: Tensor, a: Tensor, p: Tensor) -> Tensor:
    """[n] values of sum_j score(i, j) (no autograd) from a handful of elementwise ops on [n, d]: the query
    against the table's column sum c.  ComplEx (complex.py:30-39): Re<s, r, conj(o)> =
    (s_re r_re - s_im r_im) o_re + (s_re r_im + s_im r_re) o_im, linear in o ("sp": o = c) and in s ("po": s = c)."""
    c = ent.float().sum(dim=0)
    x, r = ent[a.long()].float(), rel[p.long()].float()
    if name == "distmult":
        return (x * r * c).sum(dim=1)
    h = x.shape[1] // 2
    x_re, x_im, r_re, r_im, c_re, c_im = x[:, :h], x[:, h:], r[:, :h], r[:, h:], c[:h], c[h:]
    if direction == "sp":
        return ((x_re * r_re - x_im * r_im) * c_re + (x_re * r_im + x_im * r_re) * c_im).sum(dim=1)
    return ((c_re * r_re - c_im * r_im) * x_re + (c_re * r_im + c_im * r_re) * x_im).sum(dim=1)


def bce_fused(name: str, l_norm, direction: str, ent: Tensor, rel: Tensor, a: Tensor, p: Tensor, rowptr: Tensor,
              col: Tensor, offset: float, eps: float, t, fused_fn=None) -> Tensor:
    """The fused KvsAll BCE loss with label smoothing `eps` (train_KvsAll.py:260-266; loss.py:137-159 with
    bce_type None).  With x_ij = score_ij + offset and y_ij = (1 - eps) [j in labels_i] + 1/E,
        sum_j softplus(x_ij) - y_ij x_ij
          = [sum_j softplus(x_ij) - sum_{labels} x_ij]      <- kge_bce_fwd, fused, scores never written
            + eps * sum_{labels} x_ij                       <- nnz(labels) spo scores (kge_score_spo)
            - (1/E) * sum_j x_ij                            <- one [n, 1] score against the column sum.
    fused_fn: _FusedBCE (bf16 tables; the default) or _FusedBCEF32 (float32 tables)."""
    fused = (fused_fn or _FusedBCE).apply(direction, ent, rel, a, p, rowptr, col, offset, t)
    if eps == 0.0:
        return fused
    n, E = a.shape[0], ent.shape[0]
    cnt = (rowptr[1:] - rowptr[:-1]).to(ent.device)
    col = col.to(ent.device).long()
    rows = torch.repeat_interleave(torch.arange(n, device=ent.device), cnt, output_size=col.numel())
    ar, pr = a.long()[rows], p.long()[rows]
    ent32, rel32 = ent.float(), rel.float()
    lab = (_ScoreSPO.apply(name, l_norm, ent32, rel32, ar, pr, col) if direction == "sp"
           else _ScoreSPO.apply(name, l_norm, ent32, rel32, col, pr, ar))
    s_lab = torch.zeros(n, dtype=torch.float32, device=ent.device).index_add(0, rows, lab.view(-1) + offset)
    s_all = _score_against_column_sum(name, l_norm, direction, ent, rel, a, p) + E * offset
    return fused + eps * s_lab - s_all / E


_LOSS_NODES = {"ce": (_FusedCE, _FusedCEDist, _FusedCEF32), "kl": (_FusedKL, _FusedKLDist, _FusedKLF32),
               "bce": (_FusedBCE, _FusedBCEDist, _FusedBCEF32)}


def fused_loss_rows(kind: str, direction: str, name: str, l_norm, weights, a: Tensor, p: Tensor, labels: tuple,
                    eps: float, bf16, dist, f32):
    """The [n] loss rows of the queries (a, p) ("sp": a = s; "po": a = o) from the first family of fused losses that
    takes the model's tables, or None when none does -- the one place that decides it, for KgeModel (which then composes
    the loss from the scores) and for the LibKGE plugin's models (which hand the None to the job).  kind / labels:
    "ce" (label,) -- "kl" (rowptr, col) -- "bce" (rowptr, col, offset); eps: label smoothing (0.0 for "ce").
    bf16, dist, f32: the model's _ce_tables, _ce_dist_tables, _ce_f32_tables -- asked in this order, each only when the
    ones before it returned None, and dist not under label smoothing (its uniform term is not linear in the table for a
    distance scorer).  weights: () -> (ent, rel), the parameters the gradients go to, asked once a family applies."""
    node16, node_dist, node32 = _LOSS_NODES[kind]
    t, node = bf16(), node16
    if t is None and eps == 0.0:
        t = dist()
        if t is not None:
            return node_dist.apply(direction, *weights(), a, p, *labels, *((None,) if kind == "kl" else ()), t)
    if t is None:
        t, node = f32(), node32
    if t is None:
        return None
    if kind == "ce":
        return node.apply(direction, *weights(), a, p, *labels, t)
    return (kl_fused if kind == "kl" else bce_fused)(name, l_norm, direction, *weights(), a, p, *labels, eps, t, node)


class _ScoreEmb(torch.autograd.Function):
    """Dense-embedding scoring (RelationalScorer.score_emb)."""

    @staticmethod
    def forward(ctx, name, combine, l_norm, s_emb, p_emb, o_emb):
        out = engine.score_emb(name, s_emb.detach(), p_emb.detach(), o_emb.detach(), combine, l_norm)
        ctx.meta = (name, combine, l_norm)
        ctx.save_for_backward(s_emb, p_emb, o_emb, out)
        return out

    @staticmethod
    def backward(ctx, gout):
        name, combine, l_norm = ctx.meta
        s_emb, p_emb, o_emb, out = ctx.saved_tensors
        g_s, g_p, g_o = engine.score_emb_bwd(name, s_emb, p_emb, o_emb, combine, l_norm, gout, out)
        return None, None, None, g_s, g_p, g_o
