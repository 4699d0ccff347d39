"""TrainingJob1vsAll / TrainingJobKvsAll with the kl or bce loss fused into the scoring kernel
(train.type: hip_1vsAll / hip_KvsAll) and TrainingJobNegativeSampling with the negatives of the
per-triple sampler scored by the fused gather + score kernel (train.type: hip_negative_sampling)."""
import time

import torch


def _plain_bce(loss):
    """BCEWithLogitsKgeLoss as the fused kernel computes it: bce_type None (sum over all entities),
    default BCEWithLogitsLoss arguments; returns the score offset (train.loss_arg) or None."""
    from kge.util.loss import BCEWithLogitsKgeLoss
    if not isinstance(loss, BCEWithLogitsKgeLoss) or loss._bce_type is not None:
        return None
    inner = loss._loss
    if getattr(inner, "weight", None) is not None or getattr(inner, "pos_weight", None) is not None:
        return None
    return float(loss._offset)



def _model_takes_fused_loss(model, with_dropout: bool = False) -> bool:
    """Decided ONCE per subbatch, before any backward: a decline after the first direction's
    loss.backward() would make the reference path back-propagate that direction a second time.
    with_dropout (the 1vsAll kl loss): embedder dropout in training does not decline -- the fused loss applies the
    masks itself (_FusedScoring._dropout_only)."""
    f = getattr(model, "_ce_tables", None)
    if f is not None and f() is not None:
        return True
    g = getattr(model, "_dropout_only", None)
    return bool(with_dropout and g is not None and g() is not None)


def _model_takes_dist_loss(model) -> bool:
    """The fused 1vsAll loss of the distance scorers (hip_transe / hip_rotate, `hip_1vsAll.fused_dist_loss: true`):
    decided once per subbatch like _model_takes_fused_loss.  The two one-sided calls loss_sp / loss_po; no captured
    step, no two-sided launch.  The same question for `hip_KvsAll.fused_dist_loss` (kl_loss_* / bce_loss_* per query
    type; the job adds `label_smoothing == 0`)."""
    f = getattr(model, "_ce_dist_tables", None)
    return f is not None and f() is not None


def _model_takes_f32_loss(model) -> bool:
    """The fused 1vsAll kl loss of hip_complex / hip_distmult scoring in float32 (`hip_1vsAll.fused_f32_loss: true`):
    decided once per subbatch; the two one-sided calls loss_sp / loss_po, no captured step, no two-sided launch.  The
    same question for `hip_KvsAll.fused_f32_loss` (kl_loss_* / bce_loss_* per query type, label smoothing included)."""
    f = getattr(model, "_ce_f32_tables", None)
    return f is not None and f() is not None


def _set_fused_f32_loss(job, key):
    """`<key>.fused_f32_loss` (false by default), handed to the models like `fused_dist_loss` below."""
    try:
        fused_f32 = bool(job.config.get_default(key + ".fused_f32_loss"))
    except KeyError:
        fused_f32 = False
    for m in (job.model, getattr(job.model, "_base_model", None)):
        if m is not None and hasattr(type(m), "_fused_f32_loss"):
            m._fused_f32_loss = fused_f32


def _set_fused_dist_loss(job, key):
    """`<key>.fused_dist_loss` (false by default): the models learn it here and decide per subbatch
    (_FusedScoring._ce_dist_tables); under hip_reciprocal_relations_model the base model is the one that scores."""
    try:
        fused_dist = bool(job.config.get_default(key + ".fused_dist_loss"))
    except KeyError:
        fused_dist = False
    for m in (job.model, getattr(job.model, "_base_model", None)):
        if m is not None and hasattr(type(m), "_fused_dist_loss"):
            m._fused_dist_loss = fused_dist


def _has_repeated_labels(coords) -> bool:
    """Does a batch's `label_coords` ([nnz, 2]: batch row, label) hold the same (row, label) twice?  A training split
    that repeats a triple does that: the reference's dense label row then carries a 2, while kge_kl_dist_* /
    kge_bce_dist_* (and kge_kl_f32_* / kge_bce_f32_*) take ids that are unique per row (the forward would count the id
    twice, the backward's bit mask once).  One sort of nnz keys and one host read per subbatch, on the fused_dist_loss
    and fused_f32_loss paths only."""
    if coords.shape[0] < 2:
        return False
    c = coords.long()
    key, _ = torch.sort(c[:, 0] * (c[:, 1].max() + 1) + c[:, 1])
    return bool((key[1:] == key[:-1]).any())


def _kvsall_per_type_cut(queries, coords, qtype, query_types, batch_size, row0=0):
    """A KvsAll subbatch's `label_coords` ([nnz, 2]: batch row, label; rows ascending, the whole batch's) cut into one
    CSR per query type: -> (per_type, totals) with per_type[query_type] = (query column 0, query column 1, rowptr, col)
    over the subbatch's rows of that type in batch order, totals[query_type] = its label count (one host read each).
    queries / qtype are the subbatch's, row0 its first batch row; a type without a row is left out."""
    # label ranges of all batch rows: counts -> offsets (no host sync)
    counts = torch.bincount(coords[:, 0].long(), minlength=batch_size)
    offsets = torch.zeros(batch_size + 1, dtype=torch.long, device=coords.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    per_type, totals = {}, {}
    for query_type_index, query_type in enumerate(query_types):
        examples = (qtype == query_type_index).nonzero(as_tuple=False).view(-1)
        if len(examples) == 0:
            continue
        rows = examples + row0
        cnt = counts[rows]
        rowptr = torch.zeros(len(rows) + 1, dtype=torch.long, device=cnt.device)
        torch.cumsum(cnt, 0, out=rowptr[1:])
        total = int(rowptr[-1])
        idx = torch.repeat_interleave(offsets[rows] - rowptr[:-1], cnt, output_size=total) \
            + torch.arange(total, device=cnt.device)
        per_type[query_type] = (queries[examples, 0], queries[examples, 1], rowptr, coords[idx, 1].long())
        totals[query_type] = total
    return per_type, totals


def _kvsall_pad_inputs(per_type, batch_size, dev, caps, query_types=("sp_", "_po")):
    """The per-type CSRs padded to caps = (rows per type, label entries per type): per query type (ids [rows, 2], rowptr
    [rows + 1], col [labels], weight [rows]) in one flat list, or None if a type does not fit.  A padding row is query
    (0, 0) with the single label 0 and weight 0; a real row weighs 1 / batch_size; a type without rows is all padding."""
    rows_cap, lab_cap = caps
    out = []
    for qt in query_types:
        if qt in per_type:
            q0, q1, rowptr, col = per_type[qt]
            n, nnz = len(q0), int(col.numel())
        else:
            q0 = q1 = col = torch.zeros(0, dtype=torch.long, device=dev)
            rowptr = torch.zeros(1, dtype=torch.long, device=dev)
            n, nnz = 0, 0
        pad = rows_cap - n
        if pad < 0 or nnz + pad > lab_cap:
            return None
        ids = torch.zeros(rows_cap, 2, dtype=torch.long, device=dev)
        ids[:n, 0], ids[:n, 1] = q0, q1
        rp = torch.empty(rows_cap + 1, dtype=torch.long, device=dev)
        rp[:n + 1] = rowptr
        if pad:
            rp[n + 1:] = nnz + torch.arange(1, pad + 1, device=dev)
        cl = torch.zeros(lab_cap, dtype=torch.long, device=dev)
        cl[:nnz] = col
        w = torch.zeros(rows_cap, dtype=torch.float32, device=dev)
        w[:n] = 1.0 / batch_size
        out += [ids, rp, cl, w]
    return out


def _declined_late(what):
    raise RuntimeError(f"kge_amd: {what} declined after part of the subbatch was already back-propagated "
                       "(tables or options changed inside a subbatch)")


from kge.job import Job
from kge.job.train_1vsAll import TrainingJob1vsAll
from kge.job.train_KvsAll import TrainingJobKvsAll
from kge.job.train_negative_sampling import TrainingJobNegativeSampling, S, P, O
from kge.util.loss import (BCEWithLogitsKgeLoss, KLDivWithSoftmaxKgeLoss, MarginRankingKgeLoss, SEKgeLoss,
                           SoftMarginKgeLoss)


def _optimizer_is_capturable(opt) -> bool:
    """Only optimizers whose captured step() replays correctly: kge_amd.optim.Adagrad says so itself (without lr_decay),
    HipAdam says no (host-computed bias correction would be frozen at the capture step) unless it keeps the step count
    on the device (`args: {device_step: true}`: the instance says yes), of torch's own only SGD."""
    return (all(g.get("lr_decay", 0) == 0 for g in opt.param_groups)
            and bool(getattr(opt, "graph_capturable", type(opt) is torch.optim.SGD)))


def _no_penalty(job, batch_index, batch) -> bool:
    """A penalty term back-propagates between the batch and the optimizer's step: such a job stays eager -- unless the
    terms are folded into the optimizer's pass (_fold_penalties)."""
    if getattr(job, "_folded_penalties", None):
        return True
    try:
        return len(job.model.penalty(epoch=job.epoch, batch_index=batch_index, num_batches=len(job.loader),
                                     batch=batch)) == 0
    except Exception:
        return False


def _fold_weighted_option(job) -> bool:
    """`<train.type>.fold_weighted_penalties` of the hip_1vsAll and hip_negative_sampling jobs (hip_KvsAll has the key
    too, but its captured step has no fixed `triples`: weighted terms stay eager there)."""
    try:
        kind = job.config.get("train.type")
        if kind not in ("hip_1vsAll", "hip_negative_sampling"):
            return False
        return bool(job.config.get_default(f"{kind}.fold_weighted_penalties"))
    except Exception:
        return False


def _count_weighted(job, triples):
    """The count launches of the folded WEIGHTED terms, in front of the step that reads them (inside the GraphedStep's
    function, so inside the capture, on its static `triples`): the relation embedder sees triples[:, P], the shared
    entity embedder the S and the O column (kge_model.py:607-634), both with m = len(indexes) = n -- the [n, 2] block
    the reference concatenates has len() n, so its 2n entries are divided by n (lookup_embedder.py:171).  Under
    touched_rows the same launch marks the rows."""
    for w, cols in getattr(job, "_weighted_penalties", None) or ():
        for c in cols:
            job.optimizer.count_penalty(w, triples[:, c], len(triples))


def _set_weighted_m(job, n):
    """What penalty_value divides by, for a step a replay takes (its count launches do not pass the host)."""
    for w, _cols in getattr(job, "_weighted_penalties", ()):
        job.optimizer.set_penalty_m(w, n)


def _fold_penalties(job) -> bool:
    """The embedders' UNWEIGHTED Lp / N3 penalty terms (lookup_embedder.py:122-147 through KgeModel.penalty,
    kge_model.py:603-649) folded into the pass of an optimizer that offers the penalty interface -- HipAdagrad, or a
    HipAdam with device_step: their gradient is a function of the element alone, so the optimizer adds it in registers
    and sums the term's value on the way (kge_adagrad_step_multi_penalty, kge_adam_step_multi).  A step taken
    inside `_process_batch` (a GraphedStep, replayed or eager) then carries the penalty; TrainingJob.run_epoch still
    calls `model.penalty()` afterwards, back-propagates what it gets and writes the values to the trace
    (train.py:417-436): it gets leaf scalars holding the values the step computed -- their backward is a no-op.  A
    batch whose step was NOT taken yet (subbatches, a declined fused loss) gets the reference's terms and the
    optimizer skips its folded ones for that step.

    -> True if every term of this model is folded (the job may capture its step), False if the model has no foldable
    shape (weighted terms, other embedders, other regularizers, another optimizer): nothing is changed then.

    `fold_weighted_penalties: true` (hip_1vsAll, hip_negative_sampling): WEIGHTED lp / n3 terms
    (lookup_embedder.py:148-173) are planned too -- their gradient is a function of the element and its row's count in
    the batch, which _count_weighted builds on the device in front of the step.  Declined: a
    model whose subject and object embedders differ, a model that mixes weighted and unweighted terms."""
    from kge.model import KgeModel, LookupEmbedder
    from ..optim import Adagrad as HipAdagrad, Adam as HipAdam
    model, opt = job.model, job.optimizer
    folds = isinstance(opt, HipAdagrad) or (isinstance(opt, HipAdam) and opt.device_step)
    if getattr(job, "_folded_penalties", None) is not None:
        return bool(job._folded_penalties)
    job._folded_penalties = []
    from .models import _FusedScoring  # (its penalty() is KgeModel.penalty behind a shortcut for "no terms")
    if not folds or type(model).penalty not in (KgeModel.penalty, _FusedScoring.penalty):
        return False
    pe, se, oe = model.get_p_embedder(), model.get_s_embedder(), model.get_o_embedder()
    plan, weighted = [], []
    fold_weighted = _fold_weighted_option(job)
    for emb, times in ((pe, 1.0),) + (((se, 2.0),) if se is oe else ((se, 1.0), (oe, 1.0))):
        if type(emb).penalty is not LookupEmbedder.penalty:
            return False
        if emb.regularize == "" or emb.get_option("regularize_weight") == 0.0:
            continue
        is_weighted = bool(emb.get_option("regularize_args.weighted"))
        if emb.regularize not in ("lp", "n3") or (is_weighted and not fold_weighted):
            return False
        if is_weighted:
            if emb.regularize == "n3" and emb.space != "complex":
                return False  # (the reference's weighted n3 on a real space is the SIGNED x ** 3: lookup_embedder.py:158)
            if se is not oe:
                return False  # (two entity embedders: each sees one column; not planned)
            times = 1.0       # (the S and O indexes are one vector: kge_model.py:612-621)
            weighted.append((emb._embeddings.weight, (P,) if emb is pe else (S, O)))
        if emb.regularize == "n3":
            p, kind = 3, ("n3_complex" if emb.space == "complex" else "lp")
        else:
            p = emb.get_option("regularize_args.p") if emb.has_option("regularize_args.p") else 2
            kind = "lp"
        if p not in (1, 2, 3) or float(p) != int(p):
            return False
        w = emb._embeddings.weight
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
            return False
        if kind == "n3_complex" and w.shape[1] % 8 != 0:
            return False
        if not any(w is q for g in opt.param_groups for q in g["params"]):
            return False
        plan.append((emb, w, kind, int(p), float(emb._get_regularize_weight()), times))
    if not plan:
        return False  # (nothing to fold: _no_penalty's own check decides)
    if weighted and len(weighted) != len(plan):
        return False  # (weighted and unweighted terms in one model: not planned)
    is_w = {id(w) for w, _cols in weighted}
    for emb, w, kind, p, weight, times in plan:
        if id(w) in is_w:
            opt.set_penalty(w, kind, p, weight, times, weighted=True)
        else:
            opt.set_penalty(w, kind, p, weight, times)
    job._folded_penalties = plan
    job._weighted_penalties = weighted
    reference_penalty = model.penalty

    def penalty(**kwargs):
        if job._skip_optimizer_step:  # the step -- with the terms' gradient in it -- is taken: hand over its values
            return [(f"{emb.configuration_key}.L{p}_penalty", opt.penalty_value(w).detach().requires_grad_(True))
                    for emb, w, kind, p, weight, times in plan]
        opt.skip_penalties_once()
        return reference_penalty(**kwargs)
    model.penalty = penalty
    return True


def _graphed_step_of(job, loss_fn):
    """kge_amd.train_graph.GraphedStep over `loss_fn` and the job's optimizer.  TrainingJob.run_epoch
    (kge/job/train.py:452-474) calls optimizer.step() itself after the batch: a batch that went through the GraphedStep
    (replayed or eager) has taken that step already, so the job's optimizer skips exactly that one call
    (`job._skip_optimizer_step`)."""
    from kge_amd.train_graph import GraphedStep
    opt = job.optimizer
    # (a job may build a second GraphedStep -- hip_KvsAll when its capacities grow --: always around the optimizer's OWN step)
    real_step = getattr(job, "_real_optimizer_step", None) or opt.step
    job._real_optimizer_step = real_step

    class _Opt:  # what GraphedStep needs of the optimizer, with the REAL step
        param_groups = opt.param_groups
        zero_grad = staticmethod(opt.zero_grad)
        step = staticmethod(real_step)
        graph_capturable = True  # (the caller checked the real optimizer: _optimizer_is_capturable)
        after_graph_replay = staticmethod(getattr(opt, "after_graph_replay", lambda params: None))
        # (None: GraphedStep takes the parameters that have a .grad; HipAdagrad names the touched-row ones too)
        stepped_params = staticmethod(opt.stepped_params) if callable(getattr(opt, "stepped_params", None)) else None

    def step_or_skip(*a, **k):
        if job._skip_optimizer_step:
            job._skip_optimizer_step = False
            opt._opt_called = True  # (what a learning-rate scheduler's wrapper of step() records)
            return None
        return real_step(*a, **k)
    if hasattr(real_step, "_wrapped_by_lr_sched"):  # torch's schedulers look for their mark on step()
        step_or_skip._wrapped_by_lr_sched = True
    opt.step = step_or_skip
    return GraphedStep(loss_fn, _Opt, warmup=2)


class _CudaOomText:
    """TrainingJob.run_epoch halves `train.subbatch_size` when a batch fails with a RuntimeError whose text contains
    "CUDA out of memory" (train.subbatch_auto_tune, kge/job/train.py:384-413).  On ROCm torch's allocator says "HIP out
    of memory" -- for its own allocations as for ours -- and the tuner never fires.  The hip_* jobs re-raise any
    out-of-memory error of a batch under the text the trainer matches (error conventions)."""

    def _process_batch(self, batch_index, batch):
        try:
            return super()._process_batch(batch_index, batch)
        except torch.OutOfMemoryError as e:
            if "CUDA out of memory" in str(e):
                raise
            raise RuntimeError("CUDA out of memory (ROCm: " + str(e) + ")") from e


class HipTrainingJob1vsAll(_CudaOomText, TrainingJob1vsAll):
    """Overrides only `_process_subbatch` (train_1vsAll.py:48-92).  With `train.loss: kl` and a
    model that offers `loss_sp` / `loss_po` (HipComplEx / HipDistMult scoring in bfloat16), the
    [n, E] score matrix of each direction is never written: one kernel produces the per-row
    cross entropy (kge_ce_fwd), its backward recomputes the tiles (kge_ce_bwd).  Anything else
    (other losses, float32 scoring, dropout, other models) runs the reference's code."""

    def __init__(self, config, dataset, parent_job=None, model=None, forward_only=False):
        super().__init__(config, dataset, parent_job, model=model, forward_only=forward_only)
        self._graph_step = None       # kge_amd.train_graph.GraphedStep, built at the first batch that qualifies
        self._graph_step_ok = None    # decided at the first batch (None: not yet)
        self._skip_optimizer_step = False
        _set_fused_dist_loss(self, "hip_1vsAll")
        _set_fused_f32_loss(self, "hip_1vsAll")
        if self.__class__ == HipTrainingJob1vsAll:
            for f in Job.job_created_hooks:
                f(self)

    # ---- hip_1vsAll.graph_step: forward + backward + optimizer.step of a full batch as one hipGraph replay.
    # TrainingJob.run_epoch (kge/job/train.py:452-474) calls optimizer.step() itself after the batch: the replay has
    # taken that step already, so the job's optimizer skips exactly that one call.
    def _graph_step_for(self, batch_index, batch, subbatch_slice):
        if self._graph_step_ok is False or self.is_forward_only:
            return None
        if self._graph_step_ok is None:
            ok = bool(self.config.get_default("hip_1vsAll.graph_step")) and str(self.device).startswith("cuda")
            ok = ok and _model_takes_fused_loss(self.model) and hasattr(self.model, "loss_sp_po")
            ok = ok and not _model_takes_dist_loss(self.model)  # (no captured step for the distance scorers)
            ok = ok and _optimizer_is_capturable(self.optimizer)
            ok = ok and (_fold_penalties(self) or _no_penalty(self, batch_index, batch))
            self._graph_step_ok = ok
            if ok:
                # the batch goes in as ONE tensor (one copy into the static buffer per replay, not three); the captured
                # batches all have the size of the first (another size runs eagerly), so 1 / batch size is a constant
                loss = ((lambda t: self.model.loss_sp_po_sum(t[:, 0], t[:, 1], t[:, 2], 1.0 / len(t)))
                        if hasattr(self.model, "loss_sp_po_sum")
                        else (lambda t: self.model.loss_sp_po(t[:, 0], t[:, 1], t[:, 2]).sum() / len(t)))
                if getattr(self, "_weighted_penalties", None):  # (fold_weighted_penalties: the counts, then the step)
                    plain = loss
                    loss = lambda t: (_count_weighted(self, t), plain(t))[1]
                self._graph_step = _graphed_step_of(self, loss)
        if not self._graph_step_ok:
            return None
        n = len(batch["triples"])
        sl = subbatch_slice
        whole = sl.start in (0, None) and (sl.stop is None or sl.stop >= n) and sl.step in (1, None)
        return self._graph_step if whole and _model_takes_fused_loss(self.model) else None

    def _process_subbatch_bce(self, batch_index, batch, subbatch_slice, result, offset):
        """train.loss: bce -- every triple's (s, p) row has the single label o (and (p, o) the label s):
        kge_bce_fwd with a one-entry-per-row CSR."""
        batch_size = result.size
        result.prepare_time -= time.time()
        triples = batch["triples"][subbatch_slice].to(self.device)
        rowptr = torch.arange(len(triples) + 1, dtype=torch.long, device=triples.device)
        result.prepare_time += time.time()
        for rows_fn in (lambda: self.model.bce_loss_sp(triples[:, 0], triples[:, 1], rowptr, triples[:, 2], offset),
                        lambda: self.model.bce_loss_po(triples[:, 1], triples[:, 2], rowptr, triples[:, 0], offset)):
            result.forward_time -= time.time()
            rows = rows_fn()
            if rows is None:
                _declined_late("bce_loss_sp / bce_loss_po")
            loss_value = rows.sum() / batch_size
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            result.backward_time -= time.time()
            if not self.is_forward_only:
                loss_value.backward()
            result.backward_time += time.time()

    def _process_subbatch(self, batch_index, batch, subbatch_slice, result):
        kl = isinstance(self.loss, KLDivWithSoftmaxKgeLoss) and hasattr(self.model, "loss_sp")
        takes = _model_takes_fused_loss(self.model, with_dropout=kl)
        offset = _plain_bce(self.loss)
        bce = offset is not None and hasattr(self.model, "bce_loss_sp")
        # hip_1vsAll.fused_dist_loss: loss_sp, then loss_po (kl); bce_loss_sp, then bce_loss_po (bce)
        dist = (kl or bce) and not takes and _model_takes_dist_loss(self.model)
        # hip_1vsAll.fused_f32_loss (kl only): the same two one-sided calls
        dist = dist or (kl and not takes and _model_takes_f32_loss(self.model))
        if not takes and not dist:
            return super()._process_subbatch(batch_index, batch, subbatch_slice, result)
        if bce:
            if not dist and not _model_takes_fused_loss(self.model):  # (the bce loss has no dropout form)
                return super()._process_subbatch(batch_index, batch, subbatch_slice, result)
            return self._process_subbatch_bce(batch_index, batch, subbatch_slice, result, offset)
        fused = kl
        if not fused:
            return super()._process_subbatch(batch_index, batch, subbatch_slice, result)
        batch_size = result.size
        if hasattr(self.model, "loss_sp_po") and not dist:
            gs = self._graph_step_for(batch_index, batch, subbatch_slice)
            if gs is not None and gs.enabled:
                result.forward_time -= time.time()
                # the batch as the loader made it (a host tensor): GraphedStep copies it host-to-device straight into the
                # captured step's input buffer -- no device-side hop in front of the replay
                _set_weighted_m(self, len(batch["triples"][subbatch_slice]))
                loss_value = gs(batch["triples"][subbatch_slice])  # (whole batch: len(triples) == batch_size)
                self._skip_optimizer_step = True  # (eager or replayed: the step is taken)
                result.avg_loss += loss_value.item()
                result.forward_time += time.time()
                return
        result.prepare_time -= time.time()
        triples = batch["triples"][subbatch_slice].to(self.device)
        result.prepare_time += time.time()
        if hasattr(self.model, "loss_sp_po") and not dist:
            # both directions from one scoring launch and one pair of gradient products; the sum of
            # the two losses is back-propagated once (the reference does it in two passes:
            # the same gradients, accumulated)
            result.forward_time -= time.time()
            if hasattr(self.model, "loss_sp_po_sum"):  # the sum (and its gradient) inside the loss kernels' launches
                loss_value = self.model.loss_sp_po_sum(triples[:, 0], triples[:, 1], triples[:, 2], 1.0 / batch_size)
                if loss_value is None:
                    _declined_late("loss_sp_po_sum")
            else:
                rows = self.model.loss_sp_po(triples[:, 0], triples[:, 1], triples[:, 2])
                if rows is None:
                    _declined_late("loss_sp_po")
                loss_value = rows.sum() / batch_size
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            result.backward_time -= time.time()
            if not self.is_forward_only:
                loss_value.backward()
            result.backward_time += time.time()
            return
        for loss_rows_fn in (lambda: self.model.loss_sp(triples[:, 0], triples[:, 1], triples[:, 2]),
                             lambda: self.model.loss_po(triples[:, 1], triples[:, 2], triples[:, 0])):
            result.forward_time -= time.time()
            rows = loss_rows_fn()
            if rows is None:
                _declined_late("loss_sp / loss_po")
            loss_value = rows.sum() / batch_size
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            result.backward_time -= time.time()
            if not self.is_forward_only:
                loss_value.backward()
            result.backward_time += time.time()


class HipTrainingJobKvsAll(_CudaOomText, TrainingJobKvsAll):
    """Overrides only `_process_subbatch` (train_KvsAll.py:216-294).  With `train.loss: kl` or `bce`
    (plain: bce_type None), with or without `KvsAll.label_smoothing`, and a model
    that offers `kl_loss_sp` / `kl_loss_po` (`bce_loss_sp` / `bce_loss_po`), the sp_ and _po queries of a
    subbatch get their loss from one fused kernel each (kge_kl_fwd / kge_kl_weighted_fwd /
    kge_bce_fwd: scores never written; labels as a CSR cut out of the batch's `label_coords`); s_o
    queries and every other configuration run the reference's code.  `hip_KvsAll.fused_dist_loss: true`: hip_transe /
    hip_rotate on float32 tables take the same hooks without label smoothing (kge_kl_dist_* / kge_bce_dist_*), one call
    per query type, no captured step.  `hip_KvsAll.fused_f32_loss: true`: hip_complex / hip_distmult scoring in float32
    take them too, with or without label smoothing (kge_kl_f32_* / kge_bce_f32_*), again one call per query type."""

    def __init__(self, config, dataset, parent_job=None, model=None, forward_only=False):
        super().__init__(config, dataset, parent_job, model=model, forward_only=forward_only)
        self._graph_step = None       # kge_amd.train_graph.GraphedStep over padded inputs (hip_KvsAll.graph_step)
        self._graph_step_ok = None    # decided at the first batch that could take it (None: not yet)
        self._graph_caps = None       # (rows per query type, label entries per query type) the captured step holds
        self._graph_overflows = 0     # batches in a row that did not fit the capacities
        self.graph_batches = 0        # batches that went through the GraphedStep (replayed or eager)
        self._skip_optimizer_step = False
        _set_fused_dist_loss(self, "hip_KvsAll")
        _set_fused_f32_loss(self, "hip_KvsAll")
        # the batch built on the device (hip_KvsAll.device_collate, false by default: the reference's collate function);
        # the collator itself is made where the loader is (_get_collate_fun: the indexes exist by then)
        try:
            self._device_collate = bool(config.get("hip_KvsAll.device_collate"))
        except KeyError:
            self._device_collate = False
        self._collator = None
        self._inputs_hook = None      # tests: called with ("per_type" | "graph_inputs", value) per subbatch
        if self.__class__ == HipTrainingJobKvsAll:
            for f in Job.job_created_hooks:
                f(self)

    # ---- hip_KvsAll.graph_step: forward + ONE backward for both query types + optimizer.step of a whole batch as one
    # hipGraph replay (train_KvsAll.py:216-294 issues ~40 launches per batch from ~0.3 ms of Python; the kernel-level
    # step replays in 0.2 ms: bench.py roofline_train.kvsall_step).  A batch's shapes vary -- how many of its queries
    # are sp_ / _po, how many labels each has -- so the captured step works on PADDED inputs: `rows` queries per type
    # and `labels` label entries per type; a padding row is query (0, 0) with the single label 0 and weight 0 in the
    # batch loss (its loss row is finite, its gradient row exactly zero).  A batch that does not fit runs as before;
    # three such batches in a row grow the capacities and capture again.
    def _graph_inputs(self, per_type, batch_size, dev):
        """-> the eight padded input tensors of the captured step, or None if the batch does not fit."""
        return _kvsall_pad_inputs(per_type, batch_size, dev, self._graph_caps)

    def _device_graph_inputs(self, batch, subbatch_slice, batch_size, dev):
        """The same eight tensors straight from the collator's padded typed form (hip_KvsAll.device_collate); a query
        type the job does not ask is all padding, as in _kvsall_pad_inputs."""
        ex, dev_ex = batch["examples"][subbatch_slice], batch["examples_device"][subbatch_slice]
        typed = self._collator.typed(ex, caps=self._graph_caps, weight=1.0 / batch_size, device_examples=dev_ex)
        if typed is None:
            return None
        by_type = dict(zip(self.query_types, typed))
        out = []
        for qt in ("sp_", "_po"):
            if qt in by_type:
                out += list(by_type[qt][:4])
            else:
                out += _kvsall_pad_inputs({}, batch_size, dev, self._graph_caps, query_types=(qt,))
        return out

    def _device_per_type(self, batch, subbatch_slice, batch_size, rows_of):
        """per_type of _kvsall_per_type_cut from the collator's exact-size typed form: no torch op sequence, no host wait."""
        ex, dev_ex = batch["examples"][subbatch_slice], batch["examples_device"][subbatch_slice]
        typed = self._collator.typed(ex, weight=1.0 / batch_size, device_examples=dev_ex)
        return {qt: (ids[:, 0], ids[:, 1], rowptr, col)
                for qt, (ids, rowptr, col, _, _) in zip(self.query_types, typed) if qt in rows_of}

    # ---- hip_KvsAll.device_collate: the batch is built on the GPU (kge_amd.kvsall.DeviceKvsAllCollator ->
    # kge_kvsall_collate) from its example numbers instead of the reference's collate function on the host
    # (train_KvsAll.py:118-201, a Python loop over the examples) and the copy of label_coords.  The loader hands over the
    # example numbers alone; _prepare_batch copies them and fills in the reference's dictionary as device tensors, so
    # the reference's _process_subbatch / _process_batch work on it unmodified; the fused paths take their per-type CSR
    # (padded for the captured step) from the collator as well.  On a CPU job the option is ignored.
    def _get_collate_fun(self):
        if not self._device_collate or not str(self.device).startswith("cuda"):
            return super()._get_collate_fun()
        from ..kvsall import DeviceKvsAllCollator
        self._collator = DeviceKvsAllCollator(self.query_indexes, self.query_types, self.device)

        def collate(batch):
            return {"examples": torch.as_tensor(batch, dtype=torch.long)}

        return collate

    def _prepare_batch(self, batch_index, batch, result):
        if self._collator is None:
            return super()._prepare_batch(batch_index, batch, result)
        result.prepare_time -= time.time()
        ex = batch["examples"]
        dev_ex = batch["examples_device"] = ex.to(self.device)
        batch.update(self._collator.batch(ex, device_examples=dev_ex))
        result.size = len(ex)
        result.prepare_time += time.time()

    def _graph_loss(self, ids_sp, rp_sp, cl_sp, w_sp, ids_po, rp_po, cl_po, w_po):
        offset = _plain_bce(self.loss)
        rows_sp, rows_po = self.model.multilabel_loss_sp_po(
            "kl" if offset is None else "bce", ids_sp[:, 0], ids_sp[:, 1], rp_sp, cl_sp, ids_po[:, 1], ids_po[:, 0], rp_po,
            cl_po, 0.0 if offset is None else offset)
        return (rows_sp * w_sp).sum() + (rows_po * w_po).sum()

    def _graph_step_for(self, batch_index, batch, subbatch_slice, rows_of, totals):
        """The GraphedStep for this batch (made or re-made when the capacities change), or None.  rows_of / totals: the
        subbatch's rows and label entries per query type."""
        if self._graph_step_ok is False or self.is_forward_only:
            return None
        n = len(batch["queries"])
        sl = subbatch_slice
        whole = sl.start in (0, None) and (sl.stop is None or sl.stop >= n) and sl.step in (1, None)
        if not whole:
            return None
        if self._graph_step_ok is None:
            try:
                want = bool(self.config.get_default("hip_KvsAll.graph_step"))
            except KeyError:
                want = False
            ok = want and str(self.device).startswith("cuda") and hasattr(self.model, "multilabel_loss_sp_po")
            ok = ok and float(self.label_smoothing) == 0.0 and _optimizer_is_capturable(self.optimizer)
            ok = ok and (_fold_penalties(self) or _no_penalty(self, batch_index, batch))
            self._graph_step_ok = ok
        if not self._graph_step_ok:
            return None
        caps = self._graph_caps
        if caps is None or self._graph_overflows >= 3:
            # capacities from this batch with head room (the split of a batch into sp_ / _po queries is binomial, the
            # label counts follow the data's degree distribution); never below the previous ones
            need_rows = max(list(rows_of.values()) + [1])
            need_lab = max([totals[k] for k in rows_of] + [1])
            up = lambda x, m: (int(x) + m - 1) // m * m
            rows_cap = min(up(max(need_rows * 1.15 + 16, (caps or (0, 0))[0]), 32), up(n, 32))
            rows_cap = max(rows_cap, up(need_rows, 32))
            lab_cap = up(max((need_lab + rows_cap) * 1.5, (caps or (0, 0))[1]), 256)
            self._graph_caps = (rows_cap, lab_cap)
            self._graph_step = _graphed_step_of(self, self._graph_loss)
            self._graph_overflows = 0
        return self._graph_step

    def _fused_ok(self) -> bool:
        # (s_o queries -- relation targets, off by default: config-default.yaml:322-325 -- ride along: their few hundred
        # columns go through the reference's own ops below, the entity-target queries keep the fused loss)
        if isinstance(self.loss, KLDivWithSoftmaxKgeLoss):
            return hasattr(self.model, "kl_loss_sp")
        return _plain_bce(self.loss) is not None and hasattr(self.model, "bce_loss_sp")

    def _process_subbatch(self, batch_index, batch, subbatch_slice, result):
        takes = _model_takes_fused_loss(self.model)
        # hip_KvsAll.fused_dist_loss (hip_transe / hip_rotate, no label smoothing): decided once, here; the per-type loop
        # only -- no captured step, no multilabel_loss_sp_po
        dist = not takes and float(self.label_smoothing) == 0.0 and _model_takes_dist_loss(self.model)
        # (a batch with a repeated (query, label) pair -- a split that repeats a triple -- takes the composed path)
        # hip_KvsAll.fused_f32_loss (hip_complex / hip_distmult in float32, label smoothing included): the same per-type loop
        dist = dist or (not takes and _model_takes_f32_loss(self.model))
        # (with hip_KvsAll.device_collate the question is asked of the indexes, once, at set-up: conservative)
        dist = dist and self._fused_ok() and not (
            any(self._collator.repeated_labels) if self._collator is not None
            else _has_repeated_labels(batch["label_coords"]))
        if not self._fused_ok() or not (takes or dist):
            return super()._process_subbatch(batch_index, batch, subbatch_slice, result)
        batch_size = result.size
        result.prepare_time -= time.time()
        queries = batch["queries"][subbatch_slice].to(self.device)
        if self._collator is None:
            coords = batch["label_coords"]  # [nnz, 2] (batch row, label), rows ascending; on the device
            qtype = batch["query_type_indexes"][subbatch_slice].to(self.device)
            per_type, totals = _kvsall_per_type_cut(queries, coords, qtype, self.query_types, batch_size,
                                                    subbatch_slice.start or 0)
            rows_of = {k: len(v[0]) for k, v in per_type.items()}
        else:  # sizes on the host from the collator's copy of the offsets; the tensors when a path asks for them
            n_t, nnz_t = self._collator.sizes(batch["examples"][subbatch_slice])
            rows_of = {qt: int(n) for qt, n in zip(self.query_types, n_t) if n > 0}
            totals = {qt: int(z) for qt, n, z in zip(self.query_types, n_t, nnz_t) if n > 0}
            per_type = None
        result.prepare_time += time.time()
        offset, ls = _plain_bce(self.loss), float(self.label_smoothing)
        # both query types of the subbatch: their loss rows with ONE backward (two d loss / d score passes, the gradient
        # products once over all rows, no index_add / accumulation passes of autograd in between); the reference
        # back-propagates the two losses one after the other -- the same gradients, accumulated
        if (not dist and ls == 0.0 and len(rows_of) >= 1 and hasattr(self.model, "multilabel_loss_sp_po")
                and "s_o" not in self.query_types):
            gs = self._graph_step_for(batch_index, batch, subbatch_slice, rows_of, totals)
            if gs is not None and gs.enabled:
                result.prepare_time -= time.time()
                if self._collator is None:
                    inputs = self._graph_inputs(per_type, batch_size, queries.device)
                else:
                    inputs = self._device_graph_inputs(batch, subbatch_slice, batch_size, queries.device)
                result.prepare_time += time.time()
                if inputs is None:
                    self._graph_overflows += 1
                else:
                    if self._inputs_hook is not None:
                        self._inputs_hook("graph_inputs", inputs)
                    self._graph_overflows = 0
                    result.forward_time -= time.time()
                    loss_value = gs(*inputs)
                    self._skip_optimizer_step = True  # (replayed or eager: GraphedStep has taken the optimizer's step)
                    self.graph_batches += 1
                    result.avg_loss += loss_value.item()
                    result.forward_time += time.time()
                    return
        if per_type is None:
            result.prepare_time -= time.time()
            per_type = self._device_per_type(batch, subbatch_slice, batch_size, rows_of)
            result.prepare_time += time.time()
        if self._inputs_hook is not None:
            self._inputs_hook("per_type", dict(per_type))
        if "s_o" in per_type:
            # relation targets: score_so + the job's loss on the dense [n_q, R] label matrix, exactly as the reference does
            # it (train_KvsAll.py:255-258, 279-291; label smoothing is for entity targets only there, :262-266)
            q0, q1, rowptr, col = per_type.pop("s_o")
            totals.pop("s_o")
            result.forward_time -= time.time()
            nq, R = len(q0), self.dataset.num_relations()
            labels = torch.zeros(nq, R, device=q0.device)
            rws = torch.repeat_interleave(torch.arange(nq, device=q0.device), rowptr[1:] - rowptr[:-1],
                                          output_size=int(col.numel()))
            labels[rws, col] = 1.0
            loss_value = self.loss(self.model.score_so(q0, q1), labels) / batch_size
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            result.backward_time -= time.time()
            if not self.is_forward_only:
                loss_value.backward()
            result.backward_time += time.time()
        if not dist and ls == 0.0 and len(per_type) == 2 and hasattr(self.model, "multilabel_loss_sp_po"):
            result.forward_time -= time.time()
            (s_, p_sp, rp_sp, cl_sp), (p_po, o_, rp_po, cl_po) = per_type["sp_"], per_type["_po"]
            # (averaged over the batch, not the subbatch)
            loss_value = self.model.multilabel_loss_sp_po("kl" if offset is None else "bce", s_, p_sp, rp_sp, cl_sp, o_, p_po,
                                                          rp_po, cl_po, 0.0 if offset is None else offset,
                                                          sum_scale=1.0 / batch_size)
            if loss_value is None:
                _declined_late("multilabel_loss_sp_po")
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            result.backward_time -= time.time()
            if not self.is_forward_only:
                loss_value.backward()
            result.backward_time += time.time()
            return
        for query_type, (q0, q1, rowptr, col) in per_type.items():
            result.forward_time -= time.time()
            if offset is None:
                loss_rows = (self.model.kl_loss_sp(q0, q1, rowptr, col, ls) if query_type == "sp_"
                             else self.model.kl_loss_po(q0, q1, rowptr, col, ls))
            else:
                loss_rows = (self.model.bce_loss_sp(q0, q1, rowptr, col, offset, ls) if query_type == "sp_"
                             else self.model.bce_loss_po(q0, q1, rowptr, col, offset, ls))
            if loss_rows is None:
                _declined_late("kl_loss_* / bce_loss_*")
            loss_value = loss_rows.sum() / batch_size  # averaged over the batch, not the subbatch
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            result.backward_time -= time.time()
            if not self.is_forward_only:
                loss_value.backward()
            result.backward_time += time.time()


class _FusedNegativeScore:
    """Stands in for `BatchNegativeSample.score` (sampler.py:263-344) of ONE slot's sample object for the
    duration of a subbatch: the same call, the same `forward_time` / `prepare_time` attributes -- the negatives
    go to the model's `score_neg` as (positives, neg [n, K]).  Declined by the model: the sampler's own code."""

    def __init__(self, sample, slot):
        self._sample, self._slot, self._score = sample, slot, sample.score

    def __call__(self, model, indexes=None):
        smp = self._sample
        smp.forward_time = smp.prepare_time = 0.0
        smp.prepare_time -= time.time()
        neg = smp.samples(indexes)
        tri = smp.positive_triples[indexes, :] if indexes else smp.positive_triples
        smp.prepare_time += time.time()
        smp.forward_time -= time.time()
        scores = model.score_neg(tri[:, S], tri[:, P], tri[:, O], self._slot, neg)
        smp.forward_time += time.time()
        return scores if scores is not None else self._score(model, indexes=indexes)


class _FusedSharedScore:
    """Stands in for `NaiveSharedNegativeSample.score` / `DefaultSharedNegativeSample.score` (sampler.py:428-463,
    537-578) of ONE slot's shared sample object for the duration of a subbatch: the same call, the same `forward_time`
    / `prepare_time` attributes -- the shared sample goes to the model's `score_neg_shared` as (positives, unique ids,
    drop indexes of the positives or None, repeat columns); nothing per triple is materialised (`samples(indexes)` of
    the naive object even fails on a slice).  Declined by the model: the sampler's own code."""

    def __init__(self, sample, slot):
        self._sample, self._slot, self._score = sample, slot, sample.score

    def __call__(self, model, indexes=None):
        smp = self._sample
        smp.forward_time = smp.prepare_time = 0.0
        smp.prepare_time -= time.time()
        tri = smp.positive_triples if indexes is None else smp.positive_triples[indexes, :]
        drop = getattr(smp, "_drop_index", None)
        if drop is not None and indexes is not None:
            drop = drop[indexes]
        smp.prepare_time += time.time()
        smp.forward_time -= time.time()
        scores = model.score_neg_shared(tri[:, S], tri[:, P], tri[:, O], self._slot, smp._unique_samples, drop,
                                        smp._repeat_indexes)
        smp.forward_time += time.time()
        return scores if scores is not None else self._score(model, indexes=indexes)


class _FusedNsBce(torch.autograd.Function):
    """loss = sum of kge_ns_bce_loss's per-row terms; the kernel writes d loss / d scores in the same pass."""

    @staticmethod
    def forward(ctx, scores, kind, offset, temperature):
        from .. import engine
        rows, grad = engine.ns_bce_loss(scores, kind, offset, temperature, want_grad=True)
        ctx.save_for_backward(grad)
        return rows.sum()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


class _HipNsBceLoss:
    """Stands in for the job's BCEWithLogitsKgeLoss (`train.loss: bce | bce_mean | bce_self_adversarial`,
    kge/util/loss.py:136-189) on the [n, 1 + K] score block of a negative-sampling slot: one kernel for the loss and its
    gradient instead of ~15 launches -- and, for the self-adversarial form, instead of two torch.nonzero calls (two
    device -> host waits per slot and step).  Everything it does not recognise -- CPU tensors, index labels, a label
    matrix that is not "column 0 positive, the rest negative" (checked once per label tensor: the job builds it once
    per shape and reuses it, train_negative_sampling.py:128-137) -- goes to the reference loss it wraps."""

    def __init__(self, ref_loss):
        self.ref = ref_loss
        self.kind = {None: "bce", "mean": "bce_mean", "self_adversarial": "bce_self_adversarial"}[ref_loss._bce_type]
        self.offset = float(ref_loss._offset)
        self.temperature = float(getattr(ref_loss, "_temperature", 1.0))
        self._pattern_ok = {}
        self.fused_calls = 0

    def __getattr__(self, name):  # everything else (config, _loss, _offset, ...) is the wrapped loss's
        if name == "ref":  # not set yet (copy / pickle protocols probe attributes on a blank instance): no recursion
            raise AttributeError(name)
        return getattr(self.ref, name)

    def __call__(self, scores, labels, **kwargs):
        if not (torch.is_tensor(labels) and scores.is_cuda and scores.dim() == 2 and scores.dtype == torch.float32
                and labels.dim() == 2 and labels.shape == scores.shape and scores.shape[1] >= 2):
            return self.ref(scores, labels, **kwargs)
        key = (labels.data_ptr(), tuple(labels.shape))
        ok = self._pattern_ok.get(key)
        if ok is None:
            ok = self._pattern_ok[key] = bool((labels[:, 0] == 1).all()) and bool((labels[:, 1:] == 0).all())
        if not ok:
            return self.ref(scores, labels, **kwargs)
        self.fused_calls += 1
        return _FusedNsBce.apply(scores, self.kind, self.offset, self.temperature)


def _fusable_ns_loss(loss) -> bool:
    if not isinstance(loss, BCEWithLogitsKgeLoss) or loss._bce_type not in (None, "mean", "self_adversarial"):
        return False
    inner = loss._loss
    return getattr(inner, "weight", None) is None and getattr(inner, "pos_weight", None) is None


class _FusedNsLoss(torch.autograd.Function):
    """loss = sum of kge_ns_loss's per-row terms over a [n, 1 + K] block; the kernel writes d loss / d scores in the
    same pass."""

    @staticmethod
    def forward(ctx, scores, kind, arg):
        from .. import engine
        rows, grad = engine.ns_loss(scores, kind, arg, want_grad=True)
        ctx.save_for_backward(grad)
        return rows.sum()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


class _FusedNsLossParts(torch.autograd.Function):
    """The same on two pieces -- the positives [n] and a slot's negatives [n, K] as the scoring node returns them: no
    torch.cat in front of the loss, no split of its gradient behind it (the captured step's form)."""

    @staticmethod
    def forward(ctx, pos, neg, kind, arg, temperature):
        from .. import engine
        rows, g_pos, g_neg = engine.ns_loss_parts(pos, neg, kind, arg, temperature, want_grad=True)
        ctx.save_for_backward(g_pos, g_neg)
        ctx.pos_shape = pos.shape
        return rows.sum()

    @staticmethod
    def backward(ctx, g):
        g_pos, g_neg = ctx.saved_tensors
        return (g_pos * g).view(ctx.pos_shape), g_neg * g, None, None, None


def _other_ns_loss_kind(loss):
    """(kind, arg) of kge_ns_loss for the job's loss object if it is one of LibKGE's four negative-sampling losses
    outside the bce family with its inner torch loss(es) as the reference builds them -- reduction "sum", no weight --,
    else None (the stand-in is not installed)."""
    def plain(inner, **more):
        return (getattr(inner, "reduction", None) == "sum" and getattr(inner, "weight", None) is None
                and all(getattr(inner, k, v) == v for k, v in more.items()))
    if type(loss) is KLDivWithSoftmaxKgeLoss:
        return ("kl", 0.0) if plain(loss._klloss, log_target=False) and plain(loss._celoss) else None
    if type(loss) is MarginRankingKgeLoss:
        if not plain(loss._loss) or "negative_sampling" not in str(loss._train_type):
            return None
        return "margin_ranking", float(loss._loss.margin)
    if type(loss) is SoftMarginKgeLoss:
        return ("soft_margin", 0.0) if plain(loss._loss) else None
    if type(loss) is SEKgeLoss:
        return ("se", 0.0) if plain(loss._loss) else None
    return None


class _HipNsLoss:
    """Stands in for the job's KLDivWithSoftmaxKgeLoss / MarginRankingKgeLoss / SoftMarginKgeLoss / SEKgeLoss
    (`train.loss: kl | margin_ranking | soft_margin | se`, kge/util/loss.py:192-274) on the [n, 1 + K] score block of a
    negative-sampling slot, in the mould of _HipNsBceLoss: one kernel (kge_ns_loss) for the loss and its gradient
    instead of the reference's op sequence -- for margin ranking instead of two nonzero() calls (two device -> host
    waits per slot and step) and the positives repeated to [n K].  The margin is read from the wrapped
    torch.nn.MarginRankingLoss.  Everything it does not recognise -- CPU tensors, index labels, a label matrix that is
    not "column 0 positive, the rest negative" (checked once per label tensor) -- goes to the reference loss it wraps.
    Installed by `hip_negative_sampling.fused_other_losses: true` (false by default)."""

    def __init__(self, ref_loss):
        self.ref = ref_loss
        self.kind, self.arg = _other_ns_loss_kind(ref_loss)
        self._pattern_ok = {}
        self.fused_calls = 0

    def __getattr__(self, name):  # everything else (config, _loss, ...) is the wrapped loss's
        if name == "ref":  # not set yet (copy / pickle protocols probe attributes on a blank instance): no recursion
            raise AttributeError(name)
        return getattr(self.ref, name)

    def __call__(self, scores, labels, **kwargs):
        if not (torch.is_tensor(labels) and scores.is_cuda and scores.dim() == 2 and scores.dtype == torch.float32
                and labels.dim() == 2 and labels.shape == scores.shape and scores.shape[1] >= 2):
            return self.ref(scores, labels, **kwargs)
        key = (labels.data_ptr(), tuple(labels.shape))
        ok = self._pattern_ok.get(key)
        if ok is None:
            ok = self._pattern_ok[key] = bool((labels[:, 0] == 1).all()) and bool((labels[:, 1:] == 0).all())
        if not ok:
            return self.ref(scores, labels, **kwargs)
        self.fused_calls += 1
        return _FusedNsLoss.apply(scores, self.kind, self.arg)

    def parts(self, pos, neg):
        """The loss of a slot from the positives [n] and the slot's negatives [n, K] (float32, on the GPU) -- the label
        pattern is the caller's statement: column 0 positive, the rest negative."""
        self.fused_calls += 1
        return _FusedNsLossParts.apply(pos, neg, self.kind, self.arg, 1.0)


class HipTrainingJobNegativeSampling(_CudaOomText, TrainingJobNegativeSampling):
    """`_process_subbatch` is the reference's (train_negative_sampling.py:103-164), called unchanged: labels,
    positive scores, loss, averaging, backward and every timing key are its code.  What changes is what
    `batch["negative_samples"][slot].score` does for the subject and object slots of a model that offers
    `score_neg` (the hip_* models) when the samples are the per-triple kind (DefaultBatchNegativeSample,
    sampler.py:359-380): instead of an [n*K, 3] index tensor and three [n*K, d] gathers for score_spo
    ("triple"), or an [n, U] matrix against the unique samples ("batch" / "all"), the relation row and the
    uncorrupted entity row of each positive are read once and only the corrupted rows stream (kge_score_neg,
    SURVEY 8f N2); the backward accumulates straight into the table gradients (kge_score_neg_bwd_accum).
    Shared samples (`negative_sampling.shared: true`: NaiveSharedNegativeSample / DefaultSharedNegativeSample,
    sampler.py:383-585) of the subject and object slots go to the model's `score_neg_shared` as (unique ids, drop
    indexes, repeat columns) = kge_score_neg_shared: the U distinct target rows are staged once per workgroup and
    shared by its positives instead of n K gathered rows (the "triple" implementation TransE / RotatE are forced to)
    or a subset score matrix and ~ten indexing launches per slot ("batch"); the backward is
    kge_score_neg_shared_bwd_accum -- with `hip_negative_sampling.fused_shared: true`.  The option is false by default
    (no probe numbers exist yet: DESIGN.md section 14); false, a model without the hook or a hook that declines (CPU
    tensors, dropout, a row too wide for the kernel's tile): the sampler's own `score`.  The captured step
    (graph_step) stays off for shared samples -- their shapes vary with U --, the relation slot stays the sampler's
    code."""

    def __init__(self, config, dataset, parent_job=None, model=None, forward_only=False):
        super().__init__(config, dataset, parent_job, model=model, forward_only=forward_only)
        self.type_str = "negative_sampling"
        # the bce family of losses on a GPU: loss + gradient of a slot's score block in one kernel
        # (hip_negative_sampling.fused_loss: false = the reference's loss object, untouched)
        try:
            fused_loss = bool(config.get("hip_negative_sampling.fused_loss"))
        except KeyError:
            fused_loss = True
        if str(self.device).startswith("cuda") and _fusable_ns_loss(self.loss) and fused_loss:
            self.loss = _HipNsBceLoss(self.loss)
        # kl / margin_ranking / soft_margin / se on a GPU through kge_ns_loss (hip_negative_sampling.fused_other_losses,
        # false by default: the reference's loss object, untouched)
        try:
            fused_other = bool(config.get("hip_negative_sampling.fused_other_losses"))
        except KeyError:
            fused_other = False
        if str(self.device).startswith("cuda") and fused_other and _other_ns_loss_kind(self.loss) is not None:
            self.loss = _HipNsLoss(self.loss)
        # shared samples of the subject / object slot through kge_score_neg_shared (false: the sampler's own score)
        try:
            self._fused_shared = bool(config.get("hip_negative_sampling.fused_shared"))
        except KeyError:
            self._fused_shared = False
        # embedder dropout inside the fused triple-wise kernels (hip_negative_sampling.fused_dropout, false by default: a
        # model with active dropout is scored by the sampler's and the reference model's own code)
        try:
            fused_dropout = bool(config.get("hip_negative_sampling.fused_dropout"))
        except KeyError:
            fused_dropout = False
        if hasattr(self.model, "set_fused_dropout"):
            self.model.set_fused_dropout(fused_dropout and str(self.device).startswith("cuda"))
        # the samples of the subject / object slot drawn on the device (hip_negative_sampling.device_sampler, false by
        # default: every slot's samples come from the reference's sampler on the host)
        try:
            device_sampler = bool(config.get("hip_negative_sampling.device_sampler"))
        except KeyError:
            device_sampler = False
        self._device_sampler, self._device_slots = None, ()
        if device_sampler:
            self._setup_device_sampler()
        self._graph_step = None       # kge_amd.train_graph.GraphedStep (hip_negative_sampling.graph_step)
        self._graph_step_ok = None    # decided at the first batch
        self._graph_slots = ()
        self._graph_labels = {}
        self.graph_batches = 0        # batches that went through the GraphedStep (replayed or eager)
        self._skip_optimizer_step = False
        self.touched_rows = None           # hip_negative_sampling.touched_rows: decided at the first batch
        self._touched_weighted = False     # ... with a folded weighted term on the entity table (fold_weighted_penalties)
        self.touched_rows_declined = None  # why the dense path runs although the option is on
        if self.__class__ == HipTrainingJobNegativeSampling:
            for f in Job.job_created_hooks:
                f(self)

    # ---- hip_negative_sampling.device_sampler: the [n, K] sample blocks of the subject / object slot drawn, filtered
    # and redrawn on the GPU (kge_amd.sampler.DeviceSampler -> kge_neg_sample, one launch per slot) instead of
    # KgeSampler.sample on the host for each slot (train_negative_sampling.py:64-84; with filtering a per-row loop,
    # sampler.py:163-196, 700-752) and the copy of the blocks to the device (:86-101).  The block is wrapped in the
    # reference's own DefaultBatchNegativeSample: everything downstream sees the object it sees today.  The draw happens
    # in _prepare_batch, outside the captured step.
    def _setup_device_sampler(self):
        """Which slots qualify (none: the job is the plain one) and the sampler over the training split."""
        smp, cfg = self._sampler, self.config
        if not str(self.device).startswith("cuda") or smp.shared or not smp.with_replacement:
            return
        sampling_type = cfg.get("negative_sampling.sampling_type")
        if sampling_type not in ("uniform", "frequency"):
            return
        if smp.filtering_split != cfg.get("train.split"):  # ('' = the training split: sampler.py:34-36)
            return
        slots = tuple(slot for slot in (S, O) if int(smp.num_samples[slot]) > 0)  # (empty blocks: the reference's)
        if not slots:
            return
        from ..sampler import DeviceSampler
        seed = cfg.get("random_seed.torch")
        if seed is None or int(seed) < 0:
            seed = torch.initial_seed()
        self._device_sampler = DeviceSampler(
            self.dataset.split(cfg.get("train.split")), self.dataset.num_entities(), self.dataset.num_relations(),
            sampling_type=sampling_type, smoothing=float(cfg.get("negative_sampling.frequency.smoothing")),
            filter_s=S in slots and bool(smp.filter_positives[S]), filter_o=O in slots and bool(smp.filter_positives[O]),
            seed=int(seed), device=self.device)
        self._device_slots = slots

    def _get_collate_fun(self):
        if not self._device_slots:
            return super()._get_collate_fun()

        def collate(batch):
            """The reference's collate (train_negative_sampling.py:66-82) without the host draw of the device slots."""
            triples = self.dataset.split(self.train_split)[batch, :].long()
            negative_samples = [None if slot in self._device_slots else self._sampler.sample(triples, slot)
                                for slot in (S, P, O)]
            return {"triples": triples, "negative_samples": negative_samples}

        return collate

    def _prepare_batch(self, batch_index, batch, result):
        if not self._device_slots:
            return super()._prepare_batch(batch_index, batch, result)
        from kge.util.sampler import DefaultBatchNegativeSample
        result.prepare_time -= time.time()
        triples = batch["triples"] = batch["triples"].to(self.device)
        samples = []
        for slot, ns in enumerate(batch["negative_samples"]):
            if ns is None:  # a device slot: drawn now that the triples are on the device
                K = int(self._sampler.num_samples[slot])
                ns = DefaultBatchNegativeSample(self.config, self._sampler.configuration_key, triples, slot, K,
                                                self._device_sampler.sample(triples, slot, K))
            else:
                ns.positive_triples = triples
                ns = ns.to(self.device)
            samples.append(ns)
        batch["negative_samples"] = samples
        batch["labels"] = [None] * 3  # reuse label tensors b/w subbatches
        result.size = len(triples)
        result.prepare_time += time.time()

    # ---- hip_negative_sampling.graph_step: the whole step of a full batch -- positives, the slots' negative blocks, the
    # loss of every slot, backward, optimizer.step -- as ONE hipGraph replay (kge_amd.train_graph.GraphedStep).  Through
    # the trainer a negative-sampling batch is ~50 launches of a few microseconds each, issued by ~1 ms of Python
    # (profiles/r5_libkge_plugin_gpu.jsonl, case b); its inputs have fixed shapes: triples [n, 3], negatives [n, K].
    def _graph_step_for(self, batch_index, batch, subbatch_slice):
        if self._graph_step_ok is False or self.is_forward_only:
            return None
        if self._graph_step_ok is None:
            from kge.util.sampler import DefaultBatchNegativeSample
            try:
                want = bool(self.config.get_default("hip_negative_sampling.graph_step"))
            except KeyError:
                want = False
            ok = want and str(self.device).startswith("cuda") and hasattr(self.model, "score_neg")
            ok = ok and bool(getattr(self.model, "_fused", lambda: False)())
            slots = tuple(slot for slot in (S, O) if self._sampler.num_samples[slot] > 0)
            ok = ok and len(slots) > 0 and self._sampler.num_samples[P] <= 0
            ok = ok and all(type(batch["negative_samples"][slot]) is DefaultBatchNegativeSample for slot in slots)
            # losses that are launches only: the kl loss (log_softmax + kl_div), plain bce, the one-kernel stand-ins
            # (margin ranking only as its stand-in: the reference's form waits on two nonzero() calls)
            ok = ok and (isinstance(self.loss, (KLDivWithSoftmaxKgeLoss, _HipNsBceLoss, _HipNsLoss))
                         or (isinstance(self.loss, BCEWithLogitsKgeLoss) and self.loss._bce_type is None))
            ok = ok and _optimizer_is_capturable(self.optimizer)
            ok = ok and (_fold_penalties(self) or _no_penalty(self, batch_index, batch))
            self._graph_step_ok, self._graph_slots = ok, slots
            if ok:
                self._graph_step = _graphed_step_of(self, self._graph_loss)
        if not self._graph_step_ok:
            return None
        n = len(batch["triples"])
        sl = subbatch_slice
        whole = sl.start in (0, None) and (sl.stop is None or sl.stop >= n) and sl.step in (1, None)
        return self._graph_step if whole and self.model._fused() else None

    def _graph_loss(self, triples, *args):
        """TrainingJobNegativeSampling._process_subbatch (train_negative_sampling.py:120-163) as one function of the
        batch's tensors: per slot the [n, 1 + K] block (positives | negatives), the job's loss on it / batch size; the
        slots' losses summed (the reference back-propagates them one after the other: the same gradients, accumulated)."""
        negs, inv = args[:-1], args[-1]
        s, p, o = triples[:, S], triples[:, P], triples[:, O]
        n = triples.shape[0]
        _count_weighted(self, triples)  # (fold_weighted_penalties: the counts -- and row marks -- the step reads)
        total = None
        by_slot = dict(zip(self._graph_slots, negs))
        blocks = None
        if hasattr(self.model, "score_neg_blocks"):  # positives + both slots' blocks as one autograd node
            blocks = self.model.score_neg_blocks(s, p, o, by_slot.get(S), by_slot.get(O))
        parts = isinstance(self.loss, _HipNsLoss)  # positives + the slot's block straight into kge_ns_loss: no cat
        for slot, neg in zip(self._graph_slots, negs):
            K = neg.shape[1]
            if parts and blocks is not None:
                part = self.loss.parts(blocks[0], blocks[1 if slot == S else 2]) * inv
                total = part if total is None else total + part
                continue
            labels = self._graph_labels.get((slot, n, K))
            if labels is None:
                labels = self._graph_labels[(slot, n, K)] = torch.zeros((n, 1 + K), device=triples.device)
                labels[:, 0] = 1
            if blocks is not None:
                pos, sc = blocks[0], blocks[1 if slot == S else 2]
            else:
                pos = self.model.score_spo(s, p, o, direction="spo"[slot])
                sc = self.model.score_neg(s, p, o, slot, neg)
            if sc is None:
                _declined_late("score_neg")
            scores = torch.cat([pos.view(-1, 1), sc], dim=1)
            part = self.loss(scores, labels, num_negatives=K) * inv
            total = part if total is None else total + part
        return total

    # ---- hip_negative_sampling.touched_rows: the entity table stepped on the rows the batch touched only (DESIGN.md
    # section 25).  The step of TrainingJob.run_epoch (kge/job/train.py:452-474) pays a zeros_like(ent) fill per
    # backward node and HipAdagrad's sweep of the whole table, a batch touches n (2 + K_s + K_o) rows.  Switched on, the
    # entity table's gradient lives in a persistent buffer of HipAdagrad (enable_touched_rows), the backward nodes of
    # score_spo / score_neg / score_neg_blocks accumulate into it and mark the rows, the optimizer visits the marked
    # rows.  Decided once, at the first batch, like graph_step; anything the row step does not cover runs as before.
    def _touched_rows_why_not(self, batch):
        """None if the job qualifies, else the reason it stays on the dense path."""
        from kge.model import LookupEmbedder
        from kge.util.sampler import DefaultBatchNegativeSample
        from ..model import neg_blocks_fusable
        from ..optim import Adagrad as HipAdagrad, SparseAdam as HipSparseAdam
        from .models import _FusedScoring
        model, opt = self.model, self.optimizer
        if not str(self.device).startswith("cuda"):
            return "not a CUDA device"
        if not isinstance(model, _FusedScoring) or not model._fused():
            return "the model's fused gather + score path does not apply"
        if not isinstance(opt, (HipAdagrad, HipSparseAdam)):
            return "the optimizer is not HipAdagrad or HipSparseAdam (dense Adam moves rows without a gradient)"
        emb = model.get_s_embedder()
        w = emb._embeddings.weight
        group = next((g for g in opt.param_groups if any(q is w for q in g["params"])), None)
        if group is None or group.get("weight_decay", 0) != 0:
            return "weight_decay != 0 in the entity table's parameter group"
        if type(emb) is not LookupEmbedder or emb.dropout.p > 0:
            return "the entity embedder is not a plain LookupEmbedder without dropout"
        if not (emb.regularize == "" or emb.get_option("regularize_weight") == 0.0):
            # a WEIGHTED term touches the batch's rows only: with fold_weighted_penalties it rides in the row step --
            # provided the step of EVERY batch is the GraphedStep's (whose function counts and marks the rows): the
            # captured step was decided on (before this question is asked), and the batch is never cut into subbatches
            planned = any(q is w for q, _cols in getattr(self, "_weighted_penalties", None) or ())
            sub = self.config.get("train.subbatch_size")
            whole = (sub < 1 or sub >= self.config.get("train.batch_size")) \
                and not self.config.get("train.subbatch_auto_tune")
            if not (isinstance(opt, HipAdagrad) and planned and self._graph_step_ok is True and whole):
                return "regularize_weight > 0 on the entity embedder (a penalty term touches every row)"
        if isinstance(opt, HipSparseAdam):  # the relation table goes through a bitmap too: the same conditions
            rel = model.get_p_embedder()
            if not any(q is rel._embeddings.weight for g in opt.param_groups for q in g["params"]):
                return "the relation table is in none of the optimizer's parameter groups"
            if type(rel) is not LookupEmbedder or rel.dropout.p > 0:
                return "the relation embedder is not a plain LookupEmbedder without dropout"
            if not (rel.regularize == "" or rel.get_option("regularize_weight") == 0.0):
                return "regularize_weight > 0 on the relation embedder (a penalty term touches every row)"
            if sum(p.requires_grad for p in model.parameters()) != 2:
                return "parameters other than the two embedding tables (HipSparseAdam has no dense step)"
        if self._sampler.num_samples[P] > 0:
            return "negative samples for the relation slot"
        slots = [slot for slot in (S, O) if self._sampler.num_samples[slot] > 0]
        if not slots or not all(type(batch["negative_samples"][slot]) is DefaultBatchNegativeSample for slot in slots):
            return "not per-triple samples (DefaultBatchNegativeSample) on every active slot"
        if not neg_blocks_fusable(w, model.get_p_embedder()._embeddings.weight):
            return "not contiguous float32 tables with dim <= 1024"
        return None

    def _decide_touched_rows(self, batch):
        try:
            want = bool(self.config.get_default("hip_negative_sampling.touched_rows"))
        except KeyError:
            want = False
        from ..optim import SparseAdam as HipSparseAdam
        sparse_adam = isinstance(self.optimizer, HipSparseAdam)
        self.touched_rows = False
        if self.is_forward_only:
            return
        if not want:
            if sparse_adam:  # (no dense path to fall back to)
                raise ValueError("train.optimizer.default.type: HipSparseAdam needs hip_negative_sampling.touched_rows: "
                                 "true (it steps the rows a batch marked; it has no dense step)")
            return
        why = self._touched_rows_why_not(batch)
        if why is not None:
            self.touched_rows_declined = why
            if sparse_adam:
                raise ValueError(f"hip_negative_sampling.touched_rows with HipSparseAdam: {why}")
            self.config.log(f"hip_negative_sampling.touched_rows: the dense path runs: {why}")
            return
        pair = self.optimizer.enable_touched_rows(self.model.get_s_embedder()._embeddings.weight)
        if sparse_adam:
            self.model.set_touched_rows(pair, self.optimizer.enable_touched_rows(
                self.model.get_p_embedder()._embeddings.weight))
        else:
            self.model.set_touched_rows(pair)
        self.touched_rows = True
        w = self.model.get_s_embedder()._embeddings.weight
        self._touched_weighted = any(q is w for q, _cols in getattr(self, "_weighted_penalties", None) or ())

    def _process_subbatch(self, batch_index, batch, subbatch_slice, result):
        gs = self._graph_step_for(batch_index, batch, subbatch_slice)  # (decided first: touched_rows asks about it)
        if self.touched_rows is None:
            self._decide_touched_rows(batch)
        # (a weighted term on the touched-row step is counted and marked by the GraphedStep's function alone: if the
        # capture failed and the GraphedStep switched itself off, its eager form still takes the step)
        if gs is not None and (gs.enabled or self._touched_weighted):
            batch_size = result.size
            result.prepare_time -= time.time()
            triples = batch["triples"]
            negs = [batch["negative_samples"][slot].samples() for slot in self._graph_slots]
            inv = torch.full((), 1.0 / batch_size, device=triples.device)
            _set_weighted_m(self, len(triples))
            result.prepare_time += time.time()
            result.forward_time -= time.time()
            loss_value = gs(triples, *negs, inv)
            self.graph_batches += 1
            self._skip_optimizer_step = True  # (replayed or eager: GraphedStep has taken the optimizer's step)
            result.avg_loss += loss_value.item()
            result.forward_time += time.time()
            return
        swapped = []
        if hasattr(self.model, "score_neg"):
            from kge.util.sampler import DefaultBatchNegativeSample
            for slot in (S, O):
                smp = batch["negative_samples"][slot]
                if self._sampler.num_samples[slot] > 0 and type(smp) is DefaultBatchNegativeSample:
                    smp.score = _FusedNegativeScore(smp, slot)  # instance attribute: shadows the method
                    swapped.append(smp)
        if self._fused_shared and hasattr(self.model, "score_neg_shared"):
            from kge.util.sampler import DefaultSharedNegativeSample, NaiveSharedNegativeSample
            for slot in (S, O):
                smp = batch["negative_samples"][slot]
                if (self._sampler.num_samples[slot] > 0
                        and type(smp) in (NaiveSharedNegativeSample, DefaultSharedNegativeSample)):
                    smp.score = _FusedSharedScore(smp, slot)  # instance attribute: shadows the method
                    swapped.append(smp)
        try:
            return super()._process_subbatch(batch_index, batch, subbatch_slice, result)
        finally:
            for smp in swapped:
                del smp.score
