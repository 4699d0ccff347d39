"""KgeModel / RelationalScorer subclasses routing the hot path to libkge_amd.so."""
import torch
from torch import Tensor

from kge import Config, Dataset
from kge.model.kge_model import KgeModel, RelationalScorer
from kge.model.conve import ConvE as _RefConvE
from kge.model.conve import ConvEScorer as _RefConvEScorer
from kge.model.rescal import Rescal as _RefRescal
from kge.model.rescal import RescalScorer as _RefRescalScorer
from kge.model.rescal import rescal_set_relation_embedder_dim
from kge.model.relational_tucker3 import RelationalTucker3 as _RefRelationalTucker3
from kge.model.rotate import RotatE as _RefRotatE
from kge.model.transe import TransE as _RefTransE
from kge.model.transh import TransH as _RefTransH
from kge.model.transh import TransHScorer as _RefTransHScorer
from kge.model.transh import transh_set_relation_embedder_dim

from .. import engine
from ..model import (BF16Shadow, _FusedCE2, _FusedCE2Sum, _FusedMultiLabel2, _ScoreEmb, _ScoreNeg, _ScoreNegBlocks, _ScoreNegShared,
                     _ScorePairs, _ScoreSO, _ScoreSPO, _ScoreNegDropout, _ScoreSPODropout, DropoutClock,
                     dropout_triple_fusable, ConveNetOps, ConveRoutes, Tucker3Routes, ce_fused_dropout,
                     fused_loss_rows, neg_blocks_fusable, neg_shared_fusable, predict_filters, score_so_fusable,
                     topk_composed)


class _HipScorer(RelationalScorer):
    """score_emb of the reference scorers (complex.py:18-43, distmult.py:13-25,
    transe.py:15-37, rotate.py:20-69) on dense embeddings; `s_o` keeps the reference's
    generic fallback (kge_model.py:202-209), which lands in score_emb(..., "spo") here."""

    name = None

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None):
        super().__init__(config, dataset, configuration_key)
        self._norm = float(self.get_option("l_norm")) if self.name in ("transe", "rotate") else 1.0

    def score_emb(self, s_emb, p_emb, o_emb, combine: str):
        if not p_emb.is_cuda and combine in ("spo", "sp_", "_po"):
            # `job.device: cpu` (BASELINE configs[0], examples/toy-complex-train.yaml on CPU): there is no HIP
            # device to score on, and the class this one stands in for is right there -- the REFERENCE scorer's own
            # score_emb (complex.py:18-43, ...) on this object (it reads nothing but `_norm`).  Not the oracle.
            return self._reference_scorer().score_emb(self, s_emb, p_emb, o_emb, combine)
        if combine in ("spo", "sp_", "_po"):
            n = p_emb.size(0)
            return _ScoreEmb.apply(self.name, combine, self._norm, s_emb, p_emb, o_emb).view(n, -1)
        return super().score_emb(s_emb, p_emb, o_emb, combine)

    def _reference_scorer(self):
        from kge.model.complex import ComplExScorer
        from kge.model.distmult import DistMultScorer
        from kge.model.rotate import RotatEScorer
        from kge.model.transe import TransEScorer
        return {"complex": ComplExScorer, "distmult": DistMultScorer, "transe": TransEScorer,
                "rotate": RotatEScorer}[self.name]


class HipComplExScorer(_HipScorer):
    name = "complex"


class HipDistMultScorer(_HipScorer):
    name = "distmult"


class HipTransEScorer(_HipScorer):
    name = "transe"


class HipRotatEScorer(_HipScorer):
    name = "rotate"


class HipTransHScorer(_RefTransHScorer):
    """The scorer of hip_transh.  Dense embeddings (embedder dropout in training mode, `job.device: cpu`, other
    embedders) are scored by the reference's own score_emb (transh.py:24-82: torch operations, the [m, n, d] form) --
    the library has no TransH kernel behind kge_score_emb; the index-level calls of HipTransH never come here."""

    name = "transh"

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None):
        super().__init__(config, dataset, configuration_key)
        self._norm = float(self._norm)


class HipRescalScorer(_RefRescalScorer):
    """The scorer of hip_rescal.  Dense embeddings (embedder dropout in training mode, `job.device: cpu`, other
    embedders) are scored by the reference's own score_emb (rescal.py:14-52: bmm + mm) -- the library has no RESCAL
    kernel behind kge_score_emb; the index-level calls of HipRescal never come here."""

    name = "rescal"
    _norm = 1.0  # (the tables' l_norm: ignored by the RESCAL kernels)


class _FusedScoring:
    """Overrides of KgeModel.score_* (kge_model.py:663-789): fused gather + score when both
    embedders are plain lookup tables (no active dropout, shared entity embedder)."""

    def _fused(self) -> bool:
        from kge.model import LookupEmbedder
        se, oe, pe = self.get_s_embedder(), self.get_o_embedder(), self.get_p_embedder()
        if se is not oe or type(se) is not LookupEmbedder or type(pe) is not LookupEmbedder:
            return False
        if not se._embeddings.weight.is_cuda:  # job.device: cpu -> KgeModel.score_* with the reference scorer's arithmetic
            return False
        return not (self.training and (se.dropout.p > 0 or pe.dropout.p > 0))

    def _dropout_only(self):
        """(p_entity, p_relation) if the ONLY thing that keeps `_fused()` from holding is embedder dropout in training
        mode on float32 ComplEx / DistMult tables scored in bfloat16 -- the fused 1vsAll loss then applies the masks
        itself (kge_amd.model.ce_fused_dropout: lookup_embedder.py:64-69, 102-105) --, else None."""
        from kge.model import LookupEmbedder
        se, oe, pe = self.get_s_embedder(), self.get_o_embedder(), self.get_p_embedder()
        if se is not oe or type(se) is not LookupEmbedder or type(pe) is not LookupEmbedder:
            return None
        ent, rel = self._w()
        if not (self.training and (se.dropout.p > 0 or pe.dropout.p > 0)) or not ent.is_cuda:
            return None
        if self._scorer.name not in ("complex", "distmult") or ent.dtype != torch.float32 or ent.shape[1] not in (128, 256, 512):
            return None
        try:
            if self.get_option("score_dtype") not in ("bfloat16", "bf16"):
                return None
        except KeyError:
            return None
        return float(se.dropout.p), float(pe.dropout.p)

    def _dropout_triple(self):
        """(p_entity, p_relation) if `hip_negative_sampling.fused_dropout` was set on this model (set_fused_dropout) and
        the ONLY thing that keeps `_fused()` from holding is embedder dropout in training mode, on tables the dropout
        kernels take (float32, the four scorers, dim <= 1024): score_spo / score_neg then compute the masks inside the
        kernels (kge_score_spo_dropout / kge_score_neg_dropout; lookup_embedder.py:96-105).  Else None."""
        from kge.model import LookupEmbedder
        if not getattr(self, "_fused_dropout", False) or not self.training:
            return None
        se, oe, pe = self.get_s_embedder(), self.get_o_embedder(), self.get_p_embedder()
        if se is not oe or type(se) is not LookupEmbedder or type(pe) is not LookupEmbedder:
            return None
        ent, rel = self._w()
        p_ent, p_rel = float(se.dropout.p), float(pe.dropout.p)
        if not ent.is_cuda or not dropout_triple_fusable(self._scorer.name, ent, rel, p_ent, p_rel):
            return None
        return p_ent, p_rel

    def _next_dropout(self, probs):
        """the engine.Dropout record of the next fused dropout call: the model's seed (torch.initial_seed() at the first
        call; `dropout_seed` is settable) and a host counter incremented once per call"""
        if getattr(self, "_dropout_clock", None) is None:
            self._dropout_clock = DropoutClock(getattr(self, "dropout_seed", None))
        return self._dropout_clock.next(*probs)

    def set_fused_dropout(self, on: bool):
        """hip_negative_sampling.fused_dropout: embedder dropout inside the fused triple-wise kernels"""
        self._fused_dropout = bool(on)

    def _w(self):
        return (self.get_s_embedder()._embeddings.weight, self.get_p_embedder()._embeddings.weight)

    def set_touched_rows(self, pair, rel_pair=None):
        """hip_negative_sampling.touched_rows: `pair` = HipAdagrad.enable_touched_rows(entity table) -> (grad, bitmap),
        or None.  score_spo / score_neg / score_neg_blocks hand it to their autograd nodes while the model trains: the
        backward accumulates the entity gradient into the persistent buffer and marks the rows (kge_amd.model).
        `rel_pair` = HipSparseAdam.enable_touched_rows(relation table): the relation gradient goes the same way."""
        self._touched_rows = pair if rel_pair is None else (pair, rel_pair)

    def _touched_pair(self):
        return getattr(self, "_touched_rows", None) if self.training else None

    def penalty(self, **kwargs):
        """KgeModel.penalty (kge_model.py:603-640) first copies the batch's triples to the device -- a blocking
        host-to-device copy in every batch -- and then asks the embedders, which answer with nothing when their
        `regularize_weight` is 0 (the default; lookup_embedder.py:122-126).  In exactly that case (plain
        LookupEmbedders, no penalty configured) the result is the empty list either way; the copy is skipped
        (0.1 ms of the 0.5 ms a fused 1vsAll batch takes through the trainer).  Anything else: the reference's code."""
        from kge.model import LookupEmbedder
        for e in {id(x): x for x in (self.get_s_embedder(), self.get_o_embedder(), self.get_p_embedder())}.values():
            if type(e) is not LookupEmbedder or not (e.regularize == "" or e.get_option("regularize_weight") == 0.0):
                return super().penalty(**kwargs)
        return []

    def _fwd_tables(self):
        """`score_dtype: bfloat16` (hip_complex.yaml / hip_distmult.yaml) with float32 parameters:
        sp_/_po scores come from the bf16 matrix-core kernel on bf16 copies of the tables (re-cast
        after every optimizer step), gradients are taken w.r.t. the float32 masters."""
        ent, rel = self._w()
        if self._scorer.name not in ("complex", "distmult") or ent.dtype != torch.float32:
            return None
        try:
            want = self.get_option("score_dtype")
        except KeyError:
            return None
        if want not in ("bfloat16", "bf16"):
            return None
        if getattr(self, "_bf16_shadow", None) is None:
            self._bf16_shadow = BF16Shadow()
        return self._bf16_shadow.tables(self._scorer.name, ent, rel, self._scorer._norm)

    def score_spo(self, s: Tensor, p: Tensor, o: Tensor, direction=None) -> Tensor:
        if not self._fused():
            probs = self._dropout_triple()
            if probs is not None:
                ent, rel = self._w()
                return _ScoreSPODropout.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o,
                                              self._next_dropout(probs), self._touched_pair())
            return super().score_spo(s, p, o, direction)
        ent, rel = self._w()
        return _ScoreSPO.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o, self._touched_pair())

    def score_neg(self, s: Tensor, p: Tensor, o: Tensor, slot: int, neg: Tensor) -> Tensor:
        """[n, K] scores of the positives with slot (0 = s, 2 = o) replaced by neg[i, k]: what
        BatchNegativeSample.score returns (kge/util/sampler.py:263-306), from kge_score_neg -- the
        positives' fixed rows are read once, only the corrupted rows stream; None if the fused
        path does not apply (HipTrainingJobNegativeSampling then calls the sampler's own score)."""
        if slot not in (0, 2):
            return None
        if not self._fused():
            probs = self._dropout_triple()
            if probs is None:
                return None
            ent, rel = self._w()
            return _ScoreNegDropout.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o, int(slot), neg,
                                          self._next_dropout(probs), self._touched_pair())
        ent, rel = self._w()
        if not ent.is_cuda:
            return None
        return _ScoreNeg.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o, int(slot), neg,
                               self._touched_pair())

    def score_neg_shared(self, s: Tensor, p: Tensor, o: Tensor, slot: int, unique: Tensor, drop: Tensor = None,
                         repeat: Tensor = None):
        """[n, K] scores of the positives against a SHARED negative sample of slot 0 / 2 (unique ids, drop indexes or
        None, repeat columns): what NaiveSharedNegativeSample.score / DefaultSharedNegativeSample.score return
        (kge/util/sampler.py:428-463, 537-578), from kge_score_neg_shared -- the target rows staged once per workgroup
        and shared by its positives; None if the fused path does not apply (the job then calls the sampler's score)."""
        if not self._fused() or slot not in (0, 2):
            return None
        ent, rel = self._w()
        if not ent.is_cuda or not neg_shared_fusable(ent, s.numel()):
            return None
        return _ScoreNegShared.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o, int(slot), unique, drop,
                                     repeat)

    def score_neg_blocks(self, s: Tensor, p: Tensor, o: Tensor, neg_s: Tensor = None, neg_o: Tensor = None):
        """(positives [n], subject-slot block [n, K_s] or None, object-slot block [n, K_o] or None) as ONE autograd node
        whose backward fills one pair of table gradients (kge_amd.model._ScoreNegBlocks); None if the fused gather does
        not apply (the caller composes score_spo + score_neg)."""
        if not self._fused():
            return None
        ent, rel = self._w()
        if not neg_blocks_fusable(ent, rel):
            return None
        return _ScoreNegBlocks.apply(self._scorer.name, self._scorer._norm, ent, rel, s, p, o, neg_s, neg_o,
                                     self._touched_pair())

    def _padded(self) -> bool:
        """`padded_scores` (hip_*.yaml, default true): where no gradient is recorded -- evaluation, scoring under
        torch.no_grad() -- score_sp / score_po return the [:, :E] view of a matrix whose rows start on whole 256-byte
        lines (engine.score_pitch): what the store kernels are measured on (E is odd on most datasets: the rows of a
        contiguous [n, E] float matrix start at 4-byte granularity and every 16-byte lane store straddles sectors).
        The values are the same; a caller that needs contiguous memory calls .contiguous()."""
        if torch.is_grad_enabled():
            return False
        try:
            return bool(self.get_option("padded_scores"))
        except KeyError:
            return False

    # ---- scoring without a recorded gradient: what an UNMODIFIED EntityRankingJob (eval.type: entity_ranking) calls
    # -- score_sp_po(s, p, o, torch.arange(chunk_start, chunk_end)) per chunk, score_sp / score_po against the batch's
    # unique true answers (kge/job/eval_entity_ranking.py:143-229).
    RANGE_MIN = 1024  # subsets from this length on are checked for being a contiguous range (one host read)

    def _no_grad_call(self):
        """(tables, flags) of a scoring call under torch.no_grad(), None where a gradient is recorded.  On bf16 tables
        (ComplEx / DistMult, `score_dtype: bfloat16` or bf16 parameters) the flags carry KGE_FLAG_SPLIT_QUERY unless
        `no_grad_queries: single`: the query vector as q_hi + q_lo -- the ranks of float32 arithmetic on those tables
        (what `hip_entity_ranking.bf16_queries: split` counts), where a single rounded query vector moves 4 % of them."""
        if torch.is_grad_enabled():
            return None
        ent, rel = self._w()
        t = self._fwd_tables() or engine.Tables(self._scorer.name, ent.detach(), rel.detach(), self._scorer._norm)
        flags = None
        if t.ent.dtype == torch.bfloat16 and self._scorer.name in ("complex", "distmult"):
            try:
                single = self.get_option("no_grad_queries") == "single"
            except KeyError:
                single = False
            if not single:
                flags = int(t.flags) | engine.FLAG_SPLIT_QUERY
        return t, flags

    def _targets(self, subset):
        """The reference hands an entity chunk over as torch.arange(chunk_start, chunk_end) -- also the whole table when
        nothing is chunked.  A LISTED subset keeps the kernels that gather their target rows through the index (and, with
        split queries, the f32 chain); recognised as a contiguous range (strictly increasing, last - first == len - 1:
        one small reduction + one host read, in a loop that waits for the device several times per batch anyway) it is
        scored by the all-entities kernels on rows [start, stop) of the table (kge_index.start, include/kge_amd.h)."""
        if subset is None or not torch.is_tensor(subset) or subset.dim() != 1 or subset.numel() < self.RANGE_MIN \
                or subset.dtype not in (torch.int32, torch.int64):
            return subset
        if subset.is_cuda and torch.cuda.is_current_stream_capturing():
            return subset  # (no host read inside a capture: the listed-subset kernels)
        m = subset.numel()
        ok = ((subset[-1] - subset[0]) == m - 1) & (subset[1:] > subset[:-1]).all()
        ok, first = torch.stack((ok.to(torch.int64), subset[0].to(torch.int64))).tolist()
        E = self._w()[0].shape[0]
        if not ok or first < 0 or first + m > E:
            return subset
        return None if (first == 0 and m == E) else range(first, first + m)

    def score_sp(self, s: Tensor, p: Tensor, o: Tensor = None) -> Tensor:
        if not self._fused():
            return super().score_sp(s, p, o)
        ng = self._no_grad_call()
        if ng is not None:
            return engine.score_sp(ng[0], s, p, self._targets(o), flags=ng[1], padded=self._padded())
        ent, rel = self._w()
        return _ScorePairs.apply(self._scorer.name, self._scorer._norm, "sp", ent, rel, s, p, o,
                                 self._fwd_tables(), self._padded())

    def score_po(self, p: Tensor, o: Tensor, s: Tensor = None) -> Tensor:
        if not self._fused():
            return super().score_po(p, o, s)
        ng = self._no_grad_call()
        if ng is not None:
            return engine.score_po(ng[0], p, o, self._targets(s), flags=ng[1], padded=self._padded())
        ent, rel = self._w()
        return _ScorePairs.apply(self._scorer.name, self._scorer._norm, "po", ent, rel, o, p, s,
                                 self._fwd_tables(), self._padded())

    def score_so(self, s: Tensor, o: Tensor, p: Tensor = None) -> Tensor:
        """KgeModel.score_so (kge_model.py:727-747) from kge_score_so: what hip_KvsAll calls for `s_o` queries and the
        reference sampler for the relation slot under `negative_sampling.implementation: batch`.  The reference's own
        composition (kge_model.py:202-209) wherever the kernel does not apply (other scorers, dropout, CPU, bf16 tables
        with a recorded gradient)."""
        if not self._fused():
            return super().score_so(s, o, p)
        ent, rel = self._w()
        if not score_so_fusable(self._scorer.name, ent, rel, s.numel()):
            return super().score_so(s, o, p)
        return _ScoreSO.apply(self._scorer.name, self._scorer._norm, ent, rel, s, o, p,
                              self._touched_pair() if torch.is_grad_enabled() else None)

    # filtered top-k link prediction (kge_topk): score_sp / score_po + the masking of _filter_and_rank + torch.topk
    def _predict(self, direction: str, a: Tensor, p: Tensor, k: int, filters, keep):
        """`filters`: the sets of kge_amd.model.predict_filters (the reciprocal wrapper looks its subjects up under the
        ORIGINAL relation and scores under the reciprocal one)."""
        with torch.no_grad():
            if self._fused():
                return engine.topk(self._rank_tables(), direction, a, p, k, filters, keep)
            scores = self.score_sp(a, p) if direction == "sp_" else self.score_po(p, a)
            return topk_composed(scores, k, filters, keep)

    def predict_o(self, s: Tensor, p: Tensor, k: int, filter_index=None, keep: Tensor = None):
        """(values [n, k] float32, ids [n, k] int64): the k best objects of (s_i, p_i, ?), the known answers of
        `filter_index` (a kge_amd.eval.FilterIndex) left out except keep[i]; descending score, equal scores by
        ascending entity id, (-inf, -1) where fewer than k entities are left (kge_amd.model.KgeModel.predict_o)."""
        return self._predict("sp_", s, p, k, predict_filters(filter_index, "sp_", s, p, self._w()[0].device), keep)

    def predict_s(self, p: Tensor, o: Tensor, k: int, filter_index=None, keep: Tensor = None):
        return self._predict("_po", o, p, k, predict_filters(filter_index, "_po", o, p, self._w()[0].device), keep)

    # 1vsAll loss fused with the scoring (HipTrainingJob1vsAll; kge_ce_fwd / kge_ce_bwd)
    def _ce_tables(self):
        if not self._fused() or self._scorer.name not in ("complex", "distmult"):
            return None
        ent, rel = self._w()
        t = self._fwd_tables()
        if t is None and ent.dtype == torch.bfloat16:
            t = engine.Tables(self._scorer.name, ent.detach(), rel.detach(), self._scorer._norm)
        return t if (t is not None and ent.is_cuda and engine.ce_supported(t)) else None

    # `hip_1vsAll.fused_dist_loss: true` (set by HipTrainingJob1vsAll; false by default): the 1vsAll loss of hip_transe /
    # hip_rotate on float32 tables without an [n, E] matrix (kge_ce_dist_fwd / kge_ce_dist_bwd).
    # `hip_KvsAll.fused_dist_loss: true` (set by HipTrainingJobKvsAll): the same for the KvsAll kl and bce losses without
    # label smoothing (kge_kl_dist_* / kge_bce_dist_*); also the bce loss under hip_1vsAll.
    _fused_dist_loss = False

    def _ce_dist_tables(self):
        """float32 tables for the distance scorers' fused loss, or None (the composed path): the option on, TransE /
        RotatE with l_norm 1 or 2, `_fused()` (plain lookup embedders, no active dropout, parameters on a GPU)."""
        if not self._fused_dist_loss or not self._fused() or self._scorer.name not in ("transe", "rotate"):
            return None
        ent, rel = self._w()
        if not ent.is_cuda or ent.dtype != torch.float32 or self._scorer._norm not in (1.0, 2.0):
            return None
        t = engine.Tables(self._scorer.name, ent.detach(), rel.detach(), self._scorer._norm)
        return t if engine.ce_dist_supported(t) else None

    # `hip_1vsAll.fused_f32_loss: true` (set by HipTrainingJob1vsAll; false by default): the 1vsAll kl loss of hip_complex /
    # hip_distmult scoring in float32 without an [n, E] matrix (kge_ce_f32_fwd / kge_ce_f32_bwd).
    # `hip_KvsAll.fused_f32_loss: true` (set by HipTrainingJobKvsAll): the same for the KvsAll kl and bce losses, WITH
    # label smoothing -- these scores are linear in the target row (kge_kl_f32_* / kge_bce_f32_*).
    _fused_f32_loss = False

    def _ce_f32_tables(self):
        """float32 tables for the fused loss of ComplEx / DistMult, or None (the composed path): the option on, float32
        parameters scored in float32 (no `score_dtype: bfloat16` copies), `_fused()` (plain lookup embedders, no active
        dropout, parameters on a GPU), a layout kge_ce_f32_workspace_bytes takes (dim % 8 == 0)."""
        if not self._fused_f32_loss or not self._fused() or self._scorer.name not in ("complex", "distmult"):
            return None
        ent, rel = self._w()
        if ent.dtype != torch.float32 or self._fwd_tables() is not None:  # (`_fused()`: the parameters are on a GPU)
            return None
        t = engine.Tables(self._scorer.name, ent.detach(), rel.detach(), self._scorer._norm)
        return t if engine.ce_f32_supported(t) else None

    def _rank_tables(self):
        """The tables HipEntityRankingJob counts on (kge_score_rank_sp_po: scoring + _filter_and_rank counts in one
        kernel) -- the ones score_sp_po scores on under no_grad, so that fused and two-step counts agree bit for bit:
        the bf16 copies under `score_dtype: bfloat16`, else the parameters themselves (float32: every scorer).  None:
        no fused gather (dropout active, embedders that are not plain lookup tables, job.device cpu)."""
        if not self._fused():
            return None
        ent, rel = self._w()
        return self._fwd_tables() or engine.Tables(self._scorer.name, ent.detach(), rel.detach(), self._scorer._norm)

    def _fused_rows(self, kind: str, direction: str, a: Tensor, p: Tensor, labels: tuple, eps: float = 0.0, bf16=None):
        """kge_amd.model.fused_loss_rows on this model's tables ("sp": a = s; "po": a = o): the loss rows, or None if no
        fused path applies."""
        scorer = self._scorer  # (one Module.__getattr__, not two)
        return fused_loss_rows(kind, direction, scorer.name, scorer._norm, self._w, a, p, labels, eps,
                               bf16 or self._ce_tables, self._ce_dist_tables, self._ce_f32_tables)

    def _ce_rows(self, direction: str, a: Tensor, p: Tensor, label: Tensor):
        t = self._ce_tables()
        dp = self._dropout_only() if t is None else None
        if dp is not None:  # embedder dropout in training: the masks applied here, the fused kernels on dense rows
            ent, rel = self._w()
            return ce_fused_dropout(self._scorer.name, self._scorer._norm, direction, ent, rel, a, p, label, dp[0], dp[1])
        return self._fused_rows("ce", direction, a, p, (label,), bf16=lambda: t)

    def loss_sp(self, s: Tensor, p: Tensor, o: Tensor) -> Tensor:
        """[n] cross entropy of score_sp(s, p) against o; None if the fused path does not apply."""
        return self._ce_rows("sp", s, p, o)

    def loss_po(self, p: Tensor, o: Tensor, s: Tensor) -> Tensor:
        return self._ce_rows("po", o, p, s)

    def loss_sp_po(self, s: Tensor, p: Tensor, o: Tensor) -> Tensor:
        """[2n] loss_sp rows then loss_po rows from one pass over the batch; None if not applicable."""
        t = self._ce_tables()
        if t is None:
            if self._dropout_only() is None:
                if self._ce_dist_tables() is None and self._ce_f32_tables() is None:
                    return None
                return torch.cat((self.loss_sp(s, p, o), self.loss_po(p, o, s)))  # (float32 tables: one-sided calls)
            # independent masks per direction, as the reference's two score_* calls draw them
            return torch.cat((self.loss_sp(s, p, o), self.loss_po(p, o, s)))
        ent, rel = self._w()
        return _FusedCE2.apply(ent, rel, s, p, o, t)

    def loss_sp_po_sum(self, s: Tensor, p: Tensor, o: Tensor, scale=None) -> Tensor:
        """0-d: scale * loss_sp_po(s, p, o).sum(), summed and back-propagated inside the library's launches
        (kge_amd.model._FusedCE2Sum; the step HipTrainingJob1vsAll captures); None if not applicable."""
        t = self._ce_tables()
        if t is None:
            rows = self.loss_sp_po(s, p, o)
            if rows is None:
                return None
            return rows.sum() if scale is None else rows.sum() * scale
        ent, rel = self._w()
        return _FusedCE2Sum.apply(ent, rel, s, p, o, t, scale)

    def kl_loss_sp(self, s: Tensor, p: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor,
                   label_smoothing: float = 0.0) -> Tensor:
        """[n] KL divergence of softmax(score_sp(s, p)) from the rows' normalised (and, with
        `label_smoothing`, smoothed: train_KvsAll.py:260-266) multi-hot labels (int64 CSR); None if the
        fused path does not apply (HipTrainingJobKvsAll; kge_kl_fwd / kge_kl_weighted_fwd)."""
        return self._fused_rows("kl", "sp", s, p, (lbl_rowptr, lbl_col), float(label_smoothing))

    def kl_loss_po(self, p: Tensor, o: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor,
                   label_smoothing: float = 0.0) -> Tensor:
        return self._fused_rows("kl", "po", o, p, (lbl_rowptr, lbl_col), float(label_smoothing))

    def bce_loss_sp(self, s: Tensor, p: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor, offset: float = 0.0,
                    label_smoothing: float = 0.0):
        """[n] sum over all entities of BCEWithLogits(score_sp(s, p) + offset, (smoothed) multi-hot labels);
        None if the fused path does not apply (kge_bce_fwd)."""
        return self._fused_rows("bce", "sp", s, p, (lbl_rowptr, lbl_col, float(offset)), float(label_smoothing))

    def bce_loss_po(self, p: Tensor, o: Tensor, lbl_rowptr: Tensor, lbl_col: Tensor, offset: float = 0.0,
                    label_smoothing: float = 0.0):
        return self._fused_rows("bce", "po", o, p, (lbl_rowptr, lbl_col, float(offset)), float(label_smoothing))

    def multilabel_loss_sp_po(self, kind: str, s: Tensor, p_sp: Tensor, rowptr_sp: Tensor, col_sp: Tensor, o: Tensor,
                              p_po: Tensor, rowptr_po: Tensor, col_po: Tensor, offset: float = 0.0,
                              sum_scale: float = None):
        """(loss rows of the sp_ queries, loss rows of the _po queries) of a KvsAll subbatch -- or, with `sum_scale`,
        the 0-d sum_scale * (sum of all rows) -- with ONE backward for both types (kge_amd.model._FusedMultiLabel2: no
        label smoothing); None if the fused path does not apply."""
        t = self._ce_tables()
        if t is None:
            return None
        ent, rel = self._w()
        return _FusedMultiLabel2.apply(kind, float(offset), ent, rel, s, p_sp, rowptr_sp, col_sp, o, p_po, rowptr_po,
                                       col_po, t, sum_scale)

    def score_sp_po(self, s: Tensor, p: Tensor, o: Tensor, entity_subset: Tensor = None) -> Tensor:
        if not self._fused():
            return super().score_sp_po(s, p, o, entity_subset)
        ng = self._no_grad_call()
        if ng is not None:
            return engine.score_sp_po(ng[0], s, p, o, self._targets(entity_subset), flags=ng[1])
        return torch.cat((self.score_sp(s, p, entity_subset), self.score_po(p, o, entity_subset)), dim=1)


def _init(self, scorer, config, dataset, configuration_key, init_for_load_only):
    KgeModel.__init__(self, config=config, dataset=dataset, scorer=scorer,
                      configuration_key=configuration_key, init_for_load_only=init_for_load_only)


class HipComplEx(_FusedScoring, KgeModel):
    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        _init(self, HipComplExScorer, config, dataset, configuration_key, init_for_load_only)


class HipDistMult(_FusedScoring, KgeModel):
    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        _init(self, HipDistMultScorer, config, dataset, configuration_key, init_for_load_only)


class HipTransE(_FusedScoring, _RefTransE):
    """Inherits prepare_job (forces negative_sampling.implementation=triple, transe.py:58-68)."""

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        _init(self, HipTransEScorer, config, dataset, configuration_key, init_for_load_only)


class HipTransH(_FusedScoring, _RefTransH):
    """`model: hip_transh`: kge/model/transh.py with score_spo / score_sp / score_po / score_sp_po and the negative-
    sampling blocks on the fused TransH kernels (csrc/transh.hip: no [m, n, d] tensor).  The constructor repeats
    transh.py:88-106 with the HIP scorer; `penalty` (the soft constraints, transh.py:108-142) is the reference's.
    float32 tables, l_norm 1 or 2.  Entry points without a TransH kernel are never taken: predict_o / predict_s compose
    score_sp / score_po with topk_composed, shared negative samples go back to the sampler's own score, the evaluation
    job counts on the stored score matrix, and the options that select such a kernel are refused by name."""

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        self._init_configuration(config, configuration_key)
        transh_set_relation_embedder_dim(config, dataset, self.configuration_key + ".relation_embedder")
        if float(self.get_option("l_norm")) not in (1.0, 2.0):
            raise ValueError("hip_transh: l_norm must be 1 or 2 (got {})".format(self.get_option("l_norm")))
        _init(self, HipTransHScorer, config, dataset, self.configuration_key, init_for_load_only)
        self.soft_constraint_weight = self.get_option("C")

    def penalty(self, **kwargs):
        return _RefTransH.penalty(self, **kwargs)

    def _fused(self) -> bool:
        return super()._fused() and self._w()[0].dtype == torch.float32

    def __setattr__(self, name, value):
        # hip_1vsAll / hip_KvsAll switch their fused losses on by setting these attributes on the model
        if name in ("_fused_dist_loss", "_fused_f32_loss") and value:
            raise ValueError("hip_transh: {} is not supported (no TransH kernel behind the fused losses)".format(
                name.lstrip("_")))
        super().__setattr__(name, value)

    def set_touched_rows(self, pair, rel_pair=None):
        if pair is not None:
            raise ValueError("hip_transh: touched_rows is not supported")
        self._touched_rows = None

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        return None  # (no kge_score_neg_shared kernel: the job calls the sampler's own score)

    def _rank_tables(self):
        return None  # (no counting kernel: hip_entity_ranking takes the model's score_sp_po + kge_rank_counts_multi)

    def _predict(self, direction: str, a: Tensor, p: Tensor, k: int, filters, keep):
        with torch.no_grad():
            scores = self.score_sp(a, p) if direction == "sp_" else self.score_po(p, a)
            return topk_composed(scores, k, filters, keep)


class HipRescal(_FusedScoring, _RefRescal):
    """`model: hip_rescal`: kge/model/rescal.py with score_spo / score_sp / score_po / score_sp_po and the negative-
    sampling blocks on the fused RESCAL kernels (csrc/rescal.hip: the gathered mat-vec q = M_p^T s / M_p o, then the
    float32 contraction of ComplEx / DistMult).  The constructor repeats rescal.py:58-75 with the HIP scorer.  float32
    tables, entity dim <= 256.  Entry points without a RESCAL kernel are never taken: predict_o / predict_s compose
    score_sp / score_po with topk_composed, shared negative samples go back to the sampler's own score, the evaluation
    job counts on the stored score matrix, and the options that select such a kernel are refused by name."""

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        self._init_configuration(config, configuration_key)
        rescal_set_relation_embedder_dim(config, dataset, self.configuration_key + ".relation_embedder")
        _init(self, HipRescalScorer, config, dataset, self.configuration_key, init_for_load_only)

    def _fused(self) -> bool:
        w = self._w()[0]
        return super()._fused() and w.dtype == torch.float32 and w.shape[1] <= engine.RESCAL_MAX_DIM

    def __setattr__(self, name, value):
        # hip_1vsAll / hip_KvsAll switch their fused losses on by setting these attributes on the model
        if name in ("_fused_dist_loss", "_fused_f32_loss") and value:
            raise ValueError("hip_rescal: {} is not supported (no RESCAL kernel behind the fused losses)".format(
                name.lstrip("_")))
        super().__setattr__(name, value)

    def set_touched_rows(self, pair, rel_pair=None):
        if pair is not None:
            raise ValueError("hip_rescal: touched_rows is not supported")
        self._touched_rows = None

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        return None  # (no kge_score_neg_shared kernel: the job calls the sampler's own score)

    def _rank_tables(self):
        return None  # (no counting kernel: hip_entity_ranking takes the model's score_sp_po + kge_rank_counts_multi)

    def _predict(self, direction: str, a: Tensor, p: Tensor, k: int, filters, keep):
        with torch.no_grad():
            scores = self.score_sp(a, p) if direction == "sp_" else self.score_po(p, a)
            return topk_composed(scores, k, filters, keep)


class HipRelationalTucker3(Tucker3Routes, _FusedScoring, _RefRelationalTucker3):
    """`model: hip_relational_tucker3`: kge/model/relational_tucker3.py -- RESCAL whose mixing matrices are projected
    from a base relation table, M_p = (B[p] @ W^T).view(d, d) -- with the projection on kge_tucker3_project
    (csrc/tucker3.hip) and everything behind it on the RESCAL kernels of hip_rescal over (entity table, projected rows).
    The constructor repeats relational_tucker3.py:19-38 with the HIP scorer; the embedders are the reference's own
    classes (checkpoints and `penalty` are the reference's).  With a recorded gradient the relation rows come by the
    routes of kge_amd.model.Tucker3Routes ("all" when R <= n, else "batch"); without one the projected table is cached
    until a parameter changes, unless it exceeds `projected_table_max_bytes` (then the batch's rows are projected).  Entry points without a RESCAL kernel are never taken, as for hip_rescal."""

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        from kge.misc import round_to_points
        self._init_configuration(config, configuration_key)
        ent_emb_dim = self.get_option("entity_embedder.dim")
        round_ent_emb_dim_to = self.get_option("entity_embedder.round_dim_to")
        if len(round_ent_emb_dim_to) > 0:
            ent_emb_dim = round_to_points(round_ent_emb_dim_to, ent_emb_dim)
        config.set(self.configuration_key + ".entity_embedder.dim", ent_emb_dim, log=True)
        rescal_set_relation_embedder_dim(config, dataset, self.configuration_key + ".relation_embedder")
        _init(self, HipRescalScorer, config, dataset, self.configuration_key, init_for_load_only)
        try:  # (hip_relational_tucker3.yaml; absent under a wrapper's key: the default)
            self.projected_table_max_bytes = int(self.get_option("projected_table_max_bytes"))
        except KeyError:
            pass

    def _bw(self):
        pe = self.get_p_embedder()
        return pe.base_embedder._embeddings.weight, pe.projection.weight

    def _fused(self) -> bool:
        from kge.model import LookupEmbedder, Tucker3RelationEmbedder
        se, oe, pe = self.get_s_embedder(), self.get_o_embedder(), self.get_p_embedder()
        if se is not oe or type(se) is not LookupEmbedder or type(pe) is not Tucker3RelationEmbedder or \
                type(pe.base_embedder) is not LookupEmbedder:
            return False
        ent = se._embeddings.weight
        B, W = self._bw()
        if not ent.is_cuda or any(x.dtype != torch.float32 for x in (ent, B, W)):
            return False
        if ent.shape[1] > engine.RESCAL_MAX_DIM or B.shape[1] > engine.TUCKER3_MAX_BASE_DIM:
            return False
        if pe.base_embedder.normalize_p > 0:
            return False
        return not (self.training and (se.dropout.p > 0 or pe.base_embedder.dropout.p > 0 or pe.dropout > 0))

    def _w(self):
        """(entity table, projected relation table [R, d^2]): what the RESCAL paths of _FusedScoring take."""
        return self.get_s_embedder()._embeddings.weight, self.projected_table()

    def __setattr__(self, name, value):
        if name in ("_fused_dist_loss", "_fused_f32_loss") and value:
            raise ValueError("hip_relational_tucker3: {} is not supported (no RESCAL kernel behind the fused "
                             "losses)".format(name.lstrip("_")))
        super().__setattr__(name, value)

    def set_touched_rows(self, pair, rel_pair=None):
        if pair is not None:
            raise ValueError("hip_relational_tucker3: touched_rows is not supported")
        self._touched_rows = None

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        return None  # (no kge_score_neg_shared kernel: the job calls the sampler's own score)

    def _rank_tables(self):
        return None  # (no counting kernel: hip_entity_ranking takes the model's score_sp_po + kge_rank_counts_multi)

    def _predict(self, direction: str, a: Tensor, p: Tensor, k: int, filters, keep):
        with torch.no_grad():
            scores = self.score_sp(a, p) if direction == "sp_" else self.score_po(p, a)
            return topk_composed(scores, k, filters, keep)

    def predict_o(self, s: Tensor, p: Tensor, k: int, filter_index=None, keep: Tensor = None):
        dev = self.get_s_embedder()._embeddings.weight.device
        return self._predict("sp_", s, p, k, predict_filters(filter_index, "sp_", s, p, dev), keep)

    def predict_s(self, p: Tensor, o: Tensor, k: int, filter_index=None, keep: Tensor = None):
        dev = self.get_s_embedder()._embeddings.weight.device
        return self._predict("_po", o, p, k, predict_filters(filter_index, "_po", o, p, dev), keep)

    # -- with a recorded gradient: the routes (without one, _FusedScoring's calls on `_w()`: the cached table)
    def score_spo(self, s: Tensor, p: Tensor, o: Tensor, direction=None) -> Tensor:
        if not self._fused():
            return super().score_spo(s, p, o, direction)
        rel, p2, rows = self._rel(p)
        return _ScoreSPO.apply("rescal", 1.0, self.get_s_embedder()._embeddings.weight, rel, s, p2, o, None)

    def score_neg(self, s: Tensor, p: Tensor, o: Tensor, slot: int, neg: Tensor):
        if not self._fused() or slot not in (0, 2):
            return None
        rel, p2, rows = self._rel(p)
        return _ScoreNeg.apply("rescal", 1.0, self.get_s_embedder()._embeddings.weight, rel, s, p2, o, int(slot), neg,
                               None)

    def score_neg_blocks(self, s: Tensor, p: Tensor, o: Tensor, neg_s: Tensor = None, neg_o: Tensor = None):
        if not self._fused():
            return None
        rel, p2, rows = self._rel(p)
        return _ScoreNegBlocks.apply("rescal", 1.0, self.get_s_embedder()._embeddings.weight, rel, s, p2, o, neg_s,
                                     neg_o, None)

    def _table_call(self, p: Tensor) -> bool:
        """_FusedScoring's calls on `_w()` (the cached table, range targets, padded rows): no fused gather, or no gradient
        recorded and the "all" route (the table within `projected_table_max_bytes`)"""
        return not self._fused() or (not torch.is_grad_enabled() and self.route(p.numel()) == "all")

    def score_sp(self, s: Tensor, p: Tensor, o: Tensor = None) -> Tensor:
        if self._table_call(p):
            return super().score_sp(s, p, o)
        rel, p2, rows = self._rel(p)
        return _ScorePairs.apply("rescal", 1.0, "sp", self.get_s_embedder()._embeddings.weight, rel, s, p2, o, None,
                                 self._padded(), rows)

    def score_po(self, p: Tensor, o: Tensor, s: Tensor = None) -> Tensor:
        if self._table_call(p):
            return super().score_po(p, o, s)
        rel, p2, rows = self._rel(p)
        return _ScorePairs.apply("rescal", 1.0, "po", self.get_s_embedder()._embeddings.weight, rel, o, p2, s, None,
                                 self._padded(), rows)

    def score_sp_po(self, s: Tensor, p: Tensor, o: Tensor, entity_subset: Tensor = None) -> Tensor:
        if self._table_call(p):
            return super().score_sp_po(s, p, o, entity_subset)
        return torch.cat((self.score_sp(s, p, entity_subset), self.score_po(p, o, entity_subset)), dim=1)


class HipConvEScorer(ConveNetOps, _RefConvEScorer):
    """The scorer of hip_conve: the reference's constructor (conve.py:14-73: its modules, its shape rule, the names of
    its state_dict) with score_emb restated (kge_amd.model.ConveNetOps) so that on a GPU in float32 the contraction and
    its backward are the DistMult kernels over q' = [1 | x]; on CPU it is the reference's arithmetic in torch."""

    name = "conve"
    _norm = 1.0


class HipConvE(ConveRoutes, _FusedScoring, _RefConvE):
    """`model: hip_conve`: kge/model/conve.py with score_sp and score_spo(direction="o") on the two routes of
    kge_amd.model.ConveRoutes -- kge_conve_queries + the float32 DistMult contraction in eval mode without a recorded
    gradient, torch operations with autograd otherwise.  The constructor repeats conve.py:107-135 (the +1 dimension
    hack) with the HIP scorer.  Use it as hip_reciprocal_relations_model.base_model.type: score_po, score_sp_po and the
    other directions raise the reference's errors.  Options without a ConvE kernel are refused by name."""

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        self._init_configuration(config, configuration_key)
        for key in ("entity_embedder.dim", "relation_embedder.dim"):  # HACK to add bias terms to embeddings
            self.set_option(key, self.get_option(key) + 1)
        _init(self, HipConvEScorer(config, dataset, self.configuration_key), config, dataset, self.configuration_key,
              init_for_load_only)
        for key in ("entity_embedder.dim", "relation_embedder.dim"):  # UNDO hack
            self.set_option(key, self.get_option(key) - 1)
        self._init_routes()
        try:
            self.padded_table_max_bytes = int(self.get_option("padded_table_max_bytes"))
        except KeyError:
            pass

    def _fused(self) -> bool:
        ent, rel = self._w()
        return super()._fused() and ent.dtype == torch.float32 and rel.dtype == torch.float32

    def _conve_parts(self):
        ent, rel = self._w()
        return ent, rel, self._scorer, self._fused()

    def _torch_scores(self, s, p, o, combine):
        se, pe = self.get_s_embedder().embed(s), self.get_p_embedder().embed(p)
        if o is None:
            oe = self.get_o_embedder().embed_all()
        elif isinstance(o, range):
            oe = self.get_o_embedder().embed_all()[o.start:o.stop]
        else:
            oe = self.get_o_embedder().embed(o)
        return self._scorer.score_emb(se, pe, oe, combine)

    def score_spo(self, s: Tensor, p: Tensor, o: Tensor, direction=None) -> Tensor:
        if direction != "o":
            raise ValueError("ConvE can only score objects")
        if not self._fused():
            return KgeModel.score_spo(self, s, p, o, direction)
        return self.conve_scores(s, p, o, "spo").view(-1)

    def score_sp(self, s: Tensor, p: Tensor, o: Tensor = None) -> Tensor:
        if not self._fused():
            return KgeModel.score_sp(self, s, p, o)
        return self.conve_scores(s, p, self._targets(o) if not torch.is_grad_enabled() else o, "sp_")

    def score_po(self, p: Tensor, o: Tensor, s: Tensor = None) -> Tensor:
        return KgeModel.score_po(self, p, o, s)  # (the scorer raises: "_po" is not supported)

    def score_sp_po(self, s: Tensor, p: Tensor, o: Tensor, entity_subset: Tensor = None) -> Tensor:
        return KgeModel.score_sp_po(self, s, p, o, entity_subset)  # (likewise)

    def __setattr__(self, name, value):
        # hip_1vsAll / hip_KvsAll switch their fused losses on by setting these attributes on the model
        if name in ("_fused_dist_loss", "_fused_f32_loss") and value:
            raise ValueError("hip_conve: {} is not supported (no ConvE kernel behind the fused losses)".format(
                name.lstrip("_")))
        super().__setattr__(name, value)

    def set_touched_rows(self, pair, rel_pair=None):
        if pair is not None:
            raise ValueError("hip_conve: touched_rows is not supported")
        self._touched_rows = None

    def score_neg(self, s, p, o, slot, neg):
        raise ValueError("hip_conve: negative-sampling blocks (hip_negative_sampling's score_neg) are not supported; "
                         "use train.type: negative_sampling")

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        raise ValueError("hip_conve: negative-sampling blocks (negative_sampling.shared through score_neg_shared) are "
                         "not supported; use train.type: negative_sampling")

    def score_neg_blocks(self, s, p, o, neg_s=None, neg_o=None):
        raise ValueError("hip_conve: negative-sampling blocks (hip_negative_sampling's score_neg_blocks) are not "
                         "supported; use train.type: negative_sampling")

    def _ce_tables(self):
        return None

    def _ce_dist_tables(self):
        return None

    def _ce_f32_tables(self):
        return None

    def _dropout_only(self):
        return None

    def _rank_tables(self):
        return None  # (no counting kernel: hip_entity_ranking takes the model's score_sp_po + kge_rank_counts_multi)

    def _predict(self, direction: str, a: Tensor, p: Tensor, k: int, filters, keep):
        if direction != "sp_":
            raise Exception("Combine {} not supported in ConvE's score function".format(direction))
        with torch.no_grad():
            return topk_composed(self.score_sp(a, p), k, filters, keep)


class HipRotatE(_FusedScoring, _RefRotatE):
    """Inherits normalize_phases / prepare_job (rotate.py:103-143); the constructor repeats
    rotate.py:72-101 with the HIP scorer."""

    def __init__(self, config: Config, dataset: Dataset, configuration_key=None, init_for_load_only=False):
        self._init_configuration(config, configuration_key)
        if self.get_option("entity_embedder.dim") % 2 != 0:
            raise ValueError("RotatE requires embeddings of even dimensionality"
                             " (got {})".format(self.get_option("entity_embedder.dim")))
        if self.get_option("relation_embedder.dim") < 0:
            self.set_option("relation_embedder.dim", self.get_option("entity_embedder.dim") // 2, log=True)
        _init(self, HipRotatEScorer, config, dataset, self.configuration_key, init_for_load_only)
        self._normalize_phases = self.get_option("normalize_phases")


from kge.model.reciprocal_relations_model import ReciprocalRelationsModel as _RefReciprocal  # noqa: E402


class HipReciprocalRelationsModel(_RefReciprocal):
    """`model: hip_reciprocal_relations_model` over a hip_* base model -- the reference's wrapper
    (kge/model/reciprocal_relations_model.py: separate relation embeddings p and p + R for predicting objects and
    subjects, used by most of LibKGE's tuned 1vsAll / KvsAll configurations) with its scoring routed to the base model's
    fused INDEX-level calls.  The reference wrapper embeds the batch's rows and the whole entity table and calls
    `scorer.score_emb` on the dense rows (reciprocal_relations_model.py:84-131) -- correct over a hip_* base too, through
    the dense-row kernels and a full-table gather per call --; here
        score_po(p, o, s)        = base.score_sp(o, p + R, s)                       (reciprocal_relations_model.py:84-91)
        score_sp_po(s, p, o, E') = [base.score_sp(s, p, E') | base.score_sp(o, p + R, E')]          (:96-131)
    and the fused-loss hooks of the hip_* training jobs (loss_sp / loss_po / loss_sp_po, kl_loss_*, bce_loss_*) exist with
    the same translation: BOTH directions of a 1vsAll batch are sp_ queries of the base model -- rows (s, p | label o)
    and (o, p + R | label s) -- so `loss_sp_po` is ONE fused one-sided launch over 2 n rows, and `train.type: hip_1vsAll`
    (graph_step included) / `hip_KvsAll` run their fused paths on reciprocal models.  Where the base model's fused path
    does not apply (job.device cpu, other embedders, dropout) every call is the reference wrapper's own code.
    `eval.type: hip_entity_ranking` takes its two-step path (score_sp_po above + kge_rank_counts_multi): the counting
    kernel's second side is a _po query of ONE relation table, which a reciprocal model does not have."""

    def _R(self) -> int:
        return self.dataset.num_relations()

    def _base_fused(self) -> bool:
        b = self._base_model
        return isinstance(b, _FusedScoring) and b._fused()

    def _base_triples(self) -> bool:
        """score_spo / score_neg of the base model run fused: plain lookups, or embedder dropout inside the kernels
        (hip_negative_sampling.fused_dropout)"""
        b = self._base_model
        return self._base_fused() or (isinstance(b, _FusedScoring) and b._dropout_triple() is not None)

    def set_fused_dropout(self, on: bool):
        if hasattr(self._base_model, "set_fused_dropout"):
            self._base_model.set_fused_dropout(on)

    # ---- scores
    def score_sp(self, s: Tensor, p: Tensor, o: Tensor = None) -> Tensor:
        if not self._base_fused():
            return super().score_sp(s, p, o)
        return self._base_model.score_sp(s, p, o)

    def score_po(self, p: Tensor, o: Tensor, s: Tensor = None) -> Tensor:
        if not self._base_fused():
            return super().score_po(p, o, s)
        return self._base_model.score_sp(o, p + self._R(), s)

    def score_sp_po(self, s: Tensor, p: Tensor, o: Tensor, entity_subset: Tensor = None) -> Tensor:
        if not self._base_fused():
            return super().score_sp_po(s, p, o, entity_subset)
        b = self._base_model
        # (where no gradient is recorded: ONE range check for both calls -- a Python range passes through the base
        # model's own check untouched)
        sub = b._targets(entity_subset) if not torch.is_grad_enabled() else entity_subset
        return torch.cat((b.score_sp(s, p, sub), b.score_sp(o, p + self._R(), sub)), dim=1)

    # ---- filtered top-k link prediction: both directions are sp_ queries of the base model (as score_po above); the
    # known subjects of (?, p, o) are looked up under the ORIGINAL relation p
    def predict_o(self, s: Tensor, p: Tensor, k: int, filter_index=None, keep: Tensor = None):
        b = self._base_model
        dev = b.get_s_embedder()._embeddings.weight.device
        filters = predict_filters(filter_index, "sp_", s, p, dev)
        if isinstance(b, _FusedScoring):
            return b._predict("sp_", s, p, k, filters, keep)
        with torch.no_grad():
            return topk_composed(self.score_sp(s, p), k, filters, keep)

    def predict_s(self, p: Tensor, o: Tensor, k: int, filter_index=None, keep: Tensor = None):
        b = self._base_model
        dev = b.get_s_embedder()._embeddings.weight.device
        filters = predict_filters(filter_index, "_po", o, p, dev)
        if isinstance(b, _FusedScoring):
            return b._predict("sp_", o, p + self._R(), k, filters, keep)
        with torch.no_grad():
            return topk_composed(self.score_po(p, o), k, filters, keep)

    def score_spo(self, s: Tensor, p: Tensor, o: Tensor, direction=None) -> Tensor:
        # (reciprocal_relations_model.py:74-82: "o" scores the triple as it stands, "s" the reversed triple with p + R)
        if not self._base_triples() or direction not in ("o", "s"):
            return super().score_spo(s, p, o, direction)
        if direction == "o":
            return self._base_model.score_spo(s, p, o, "o")
        return self._base_model.score_spo(o, p + self._R(), s, "o")

    def score_neg(self, s: Tensor, p: Tensor, o: Tensor, slot: int, neg: Tensor):
        """[n, K] scores of the positives with slot (0 = s, 2 = o) replaced by neg[i, k] -- the hook
        HipTrainingJobNegativeSampling hands a slot's samples to (BatchNegativeSample.score, kge/util/sampler.py:263-306,
        which asks score_spo(..., direction) of this wrapper): a corrupted SUBJECT is the corrupted object of the
        reversed triple (o, p + R, s').  None: the sampler's own code."""
        b = self._base_model
        if not self._base_triples() or not hasattr(b, "score_neg"):
            return None
        if slot == 2:
            return b.score_neg(s, p, o, 2, neg)
        if slot == 0:
            return b.score_neg(o, p + self._R(), s, 2, neg)
        return None

    def score_neg_shared(self, s: Tensor, p: Tensor, o: Tensor, slot: int, unique: Tensor, drop: Tensor = None,
                         repeat: Tensor = None):
        """score_neg for a SHARED sample (unique ids, drop indexes, repeat columns; sampler.py:428-463, 537-578) with the
        same translation: a corrupted subject is the corrupted object of the reversed triple (o, p + R, s')."""
        b = self._base_model
        if not self._base_fused() or not hasattr(b, "score_neg_shared"):
            return None
        if slot == 2:
            return b.score_neg_shared(s, p, o, 2, unique, drop, repeat)
        if slot == 0:
            return b.score_neg_shared(o, p + self._R(), s, 2, unique, drop, repeat)
        return None

    # ---- the fused-loss hooks of HipTrainingJob1vsAll / HipTrainingJobKvsAll (train_job.py)
    def _ce_tables(self):
        f = getattr(self._base_model, "_ce_tables", None)
        return f() if f is not None else None

    def _dropout_only(self):
        f = getattr(self._base_model, "_dropout_only", None)
        return f() if f is not None else None

    def _ce_dist_tables(self):
        f = getattr(self._base_model, "_ce_dist_tables", None)
        return f() if f is not None else None

    def _ce_f32_tables(self):
        f = getattr(self._base_model, "_ce_f32_tables", None)
        return f() if f is not None else None

    def loss_sp(self, s: Tensor, p: Tensor, o: Tensor) -> Tensor:
        return self._base_model.loss_sp(s, p, o)

    def loss_po(self, p: Tensor, o: Tensor, s: Tensor) -> Tensor:
        return self._base_model.loss_sp(o, p + self._R(), s)

    def loss_sp_po(self, s: Tensor, p: Tensor, o: Tensor) -> Tensor:
        """[2n] loss rows, the sp_ queries first: one fused launch over the 2 n sp_ queries of the base model."""
        return self._base_model.loss_sp(torch.cat((s, o)), torch.cat((p, p + self._R())), torch.cat((o, s)))

    def kl_loss_sp(self, s, p, lbl_rowptr, lbl_col, label_smoothing: float = 0.0):
        return self._base_model.kl_loss_sp(s, p, lbl_rowptr, lbl_col, label_smoothing)

    def kl_loss_po(self, p, o, lbl_rowptr, lbl_col, label_smoothing: float = 0.0):
        return self._base_model.kl_loss_sp(o, p + self._R(), lbl_rowptr, lbl_col, label_smoothing)

    def bce_loss_sp(self, s, p, lbl_rowptr, lbl_col, offset: float = 0.0, label_smoothing: float = 0.0):
        return self._base_model.bce_loss_sp(s, p, lbl_rowptr, lbl_col, offset, label_smoothing)

    def bce_loss_po(self, p, o, lbl_rowptr, lbl_col, offset: float = 0.0, label_smoothing: float = 0.0):
        return self._base_model.bce_loss_sp(o, p + self._R(), lbl_rowptr, lbl_col, offset, label_smoothing)
