"""torch.optim.Adagrad / torch.optim.Adam with the update done by HIP kernels (kge_adagrad_step_multi: every dense
table of a device in one launch, kge_adagrad_step_rows for row-sparse gradients, kge_adagrad_step_touched for a table
whose backward marks the rows it touched (Adagrad.enable_touched_rows), kge_adam_step per parameter, or
kge_adam_step_multi with Adam(device_step=True): the step count on the device, one launch, capturable), optionally
maintaining the bf16 copies of the tables that mixed-precision scoring reads.  `SparseAdam`: torch.optim.SparseAdam on
the rows a backward marked (kge_sparse_adam_step_touched), the plugin's `HipSparseAdam`.

Drop-in for `torch.optim.Adagrad` (same constructor arguments, same `state_dict`: per-parameter
"step" and "sum"), so LibKGE's optimizer checkpoints load either way.  Parameters the kernel does
not cover (CPU tensors, non-float32, sparse gradients, a parameter / gradient / state tensor
whose data pointer is not 16-byte aligned) are stepped by torch's own functional Adagrad.  kge/util/optimizer.py:15-20 resolves `train.optimizer.default.type` with
`getattr(torch.optim, ...)`; the LibKGE plugin registers this class there as `HipAdagrad`.
"""
import torch
from torch.optim.adagrad import Adagrad as _TorchAdagrad
from torch.optim.adagrad import adagrad as _functional_adagrad

from . import _lib, engine

# (bf16 tensor, version of the parameter it was made from, data_ptr of the parameter's storage then),
# set on the parameter
BF16_ATTR = "_kge_bf16_copy"


def bf16_copy_of(param: torch.Tensor):
    """The optimizer-maintained bf16 copy of `param`, or None if there is none / it is stale.
    Stale = the version counter moved OR the storage was replaced: `weight.data = ...`
    (LookupEmbedder._normalize_embeddings, lookup_embedder.py:64-69, run as a post-batch hook when
    normalize.p > 0) swaps the storage without bumping the counter."""
    rec = getattr(param, BF16_ATTR, None)
    if rec is None or rec[1] != param._version or rec[2] != param.data_ptr() or rec[0].data_ptr() == 0:
        return None
    return rec[0]


class _FoldedPenalties:
    """The embedders' unweighted penalty terms inside the optimizer's own pass (kge_adagrad_step_multi_penalty,
    kge_adam_step_multi with penalty segments): what Adagrad and the device-step Adam share."""

    def _init_penalties(self):
        self._penalties = {}       # parameter -> (kind, p, gradient factor, row_dim, value factor)
        self._pen_acc = {}         # device -> float64 accumulators, one per parameter with a penalty
        self._pen_slot = {}        # parameter -> index into its device's accumulators
        self._pen_off_once = False
        self._wpen = {}            # parameter with a WEIGHTED term -> [count buffer [V] (zero between steps), m]

    def set_penalty(self, param, kind: str, p: int, weight: float, times: float = 1.0, weighted: bool = False):
        """From now on every step() adds to `param`'s gradient the gradient of
            times * weight / p * sum |x|^p                      kind "lp", p in (1, 2, 3)
            times * weight / 3 * sum |z|^3 over complex coordinates   kind "n3_complex" (z = row[c] + i row[c + dim / 2])
        (LookupEmbedder.penalty unweighted, lookup_embedder.py:122-147; `times` = 2 for an entity embedder that serves the
        subject and the object slot, kge_model.py:620-625) inside the update's own pass, and `penalty_value(param)`
        holds the term's value at the parameters the step started from.  The caller must then NOT back-propagate the
        term itself.  kind None removes it.

        weighted=True: the frequency-weighted form (lookup_embedder.py:148-173),
            weight / p / m * sum_r c_r * sum_j |x_rj|^p,  c_r = the occurrences of row r among the batch's m indexes.
        The parameter then owns a zero [rows] count buffer; before every step() the caller counts the batch's indexes
        into it with `count_penalty(param, ids, m)`, and step() leaves it zero again.  `times` must be 1: a shared
        entity embedder gets the subject and object indexes as one [n, 2] tensor (kge_model.py:612-621) whose 2n
        entries are counted and whose len(), n, is the m the reference divides by (lookup_embedder.py:171)."""
        name = f"kge_amd.optim.{type(self).__name__}"
        if kind is None:
            self._penalties.pop(param, None)
            self._wpen.pop(param, None)
        else:
            if kind not in ("lp", "n3_complex") or (kind == "lp" and p not in (1, 2, 3)):
                raise ValueError(f"{name}: no fused form of penalty {kind} p={p}")
            if not (param.is_cuda and param.dtype == torch.float32 and param.is_contiguous()):
                raise ValueError(f"{name}: fused penalties are for dense float32 GPU parameters")
            if kind == "n3_complex":
                p = 3
                if param.dim() != 2 or param.shape[1] % 8 != 0:
                    raise ValueError(f"{name}: n3_complex needs a [*, dim] table with dim % 8 == 0")
            if weighted:
                if param.dim() != 2:
                    raise ValueError(f"{name}: a weighted penalty needs a [rows, dim] table")
                if float(times) != 1.0:
                    raise ValueError(f"{name}: a weighted penalty is not doubled (count both slots' indexes instead)")
                if param not in self._wpen or self._wpen[param][0].numel() < param.shape[0]:
                    self._wpen[param] = [engine.penalty_counts(param.shape[0], param.device), 0]
            else:
                self._wpen.pop(param, None)
            self._penalties[param] = (1 if kind == "lp" else 2, int(p), float(times) * float(weight),
                                      int(param.shape[-1]), float(times) * float(weight) / float(p))
        self._pen_acc, self._pen_slot = {}, {}
        for q in self._penalties:
            acc = self._pen_acc.get(q.device)
            self._pen_slot[q] = 0 if acc is None else acc.numel()
            self._pen_acc[q.device] = torch.zeros(self._pen_slot[q] + 1, dtype=torch.float64, device=q.device)

    def has_penalties(self) -> bool:
        return bool(self._penalties)

    def skip_penalties_once(self):
        """The next step() is the plain update (the caller back-propagated the terms itself for that batch); the count
        buffers of weighted terms are zeroed by it all the same."""
        self._pen_off_once = True

    def is_weighted(self, param) -> bool:
        return param in self._wpen

    def penalty_counts(self, param) -> torch.Tensor:
        """The [rows] int32 count buffer of a weighted term (zero between steps)."""
        return self._wpen[param][0]

    def count_penalty(self, param, ids: torch.Tensor, m: int):
        """Counts `ids` (an index vector or [n, k] block, any stride: engine.penalty_count) into the weighted term's
        buffer for the next step().  `m` is len(indexes) as the reference's term divides by it: the same in every call
        of one step (the subject and the object column of a batch of n triples are two calls, BOTH with m = n: the
        reference passes them as one [n, 2] tensor, whose len() is n).  A parameter on the touched-row step has the
        rows marked too, and a SparseAdam pair is set `pending`: the next step() visits the rows and clears the counts
        whether or not a backward ran."""
        rec = self._wpen[param]
        if not 0 < int(m) < engine.WPENALTY_MAX_M:
            raise ValueError(f"kge_amd.optim.{type(self).__name__}: a weighted penalty needs 0 < m < 2^24 indexes")
        rec[1] = int(m)
        pair = getattr(self, "_touched", {}).get(param)
        engine.penalty_count(ids, rec[0], param.shape[0], None if pair is None else pair[1])
        if isinstance(pair, _TouchedRows):
            pair.pending = True

    def set_penalty_m(self, param, m: int):
        """The length of the index vector of the step about to be REPLAYED (its captured count launches do not pass
        the host): what penalty_value divides by."""
        self._wpen[param][1] = int(m)

    def penalty_value(self, param) -> torch.Tensor:
        """0-d float32 device tensor: the term's value the LAST step() saw (pre-step parameters)."""
        spec = self._penalties[param]
        factor = spec[4] / self._wpen[param][1] if param in self._wpen else spec[4]
        return (self._pen_acc[param.device][self._pen_slot[param]] * factor).to(torch.float32)

    def _begin_fold(self) -> bool:
        """Whether this step() carries the terms; if so their accumulators are cleared, if not the count buffers of
        the weighted ones are (a skipped step must leave them zero as well)."""
        fold = bool(self._penalties) and not self._pen_off_once
        if fold:
            for acc in self._pen_acc.values():
                acc.zero_()  # (a fill kernel: captured with the step)
        else:
            for rec in self._wpen.values():
                rec[0].zero_()
        return fold

    def _fold_this_step(self) -> bool:
        """_begin_fold, and ends a skip_penalties_once."""
        fold = self._begin_fold()
        self._pen_off_once = False
        return fold

    def _wpenalty_seg(self, q):
        """The kge_wpenalty_seg record of parameter `q` (kind 0 if it has no weighted term)."""
        rec = self._wpen.get(q)
        if rec is None:
            return engine.wpenalty_seg(0, 0, 0.0, 0, None, None, 0)
        if rec[1] <= 0:
            raise RuntimeError(f"kge_amd.optim.{type(self).__name__}: a weighted penalty was never counted "
                               "(count_penalty before step())")
        spec = self._penalties[q]
        return engine.wpenalty_seg(spec[0], spec[1], spec[2], spec[3],
                                   self._pen_acc[q.device].data_ptr() + 8 * self._pen_slot[q], rec[0], rec[1])

    def _penalty_segs(self, params, device):
        """The kge_penalty_seg array of one launch over `params`, or None if none of them has a term."""
        if any(q in self._wpen for q in params):
            raise RuntimeError("kge_amd.optim: a weighted term in an unweighted penalty launch")
        if not any(q in self._penalties for q in params):
            return None
        pens = []
        for q in params:
            spec = self._penalties.get(q)
            if spec is None:
                pens.append(_lib.KgePenaltySeg(0, 0, 0.0, 0, None))
            else:
                pens.append(_lib.KgePenaltySeg(spec[0], spec[1], spec[2], spec[3],
                                               self._pen_acc[device].data_ptr() + 8 * self._pen_slot[q]))
        return (_lib.KgePenaltySeg * len(pens))(*pens)


class Adagrad(_FoldedPenalties, _TorchAdagrad):
    # kge_amd.train_graph.GraphedStep: the step's launch arguments do not depend on the step count (lr_decay != 0 is
    # refused there), so a captured step() replays correctly; `after_graph_replay` keeps state["step"] -- which the
    # checkpoint carries -- counting.
    graph_capturable = True

    def after_graph_replay(self, params):
        """`params`: the parameters the captured step() updated."""
        for p in params:
            st = self.state.get(p)
            if st is not None and "step" in st:
                st["step"] += 1

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10,
                 bf16_copies: bool = False, **kw):
        """bf16_copies=True: after every step each 2-D float32 parameter carries a fresh bf16 copy
        (written by the same kernel pass) that `kge_amd.model.BF16Shadow` picks up instead of
        re-casting the table before the next scoring call."""
        kw.pop("foreach", None)
        kw.pop("fused", None)
        super().__init__(params, lr=lr, lr_decay=lr_decay, weight_decay=weight_decay,
                         initial_accumulator_value=initial_accumulator_value, eps=eps, foreach=False, **kw)
        self.bf16_copies = bool(bf16_copies)
        self._init_penalties()
        self._touched = {}   # parameter -> (persistent dense gradient [E, d], bitmap): enable_touched_rows
        self._stepped = []   # the parameters the last step() updated: stepped_params

    # ---- the step over the rows a batch touched (kge_adagrad_step_touched) ----------------------
    def enable_touched_rows(self, param):
        """From now on `param` -- a 2-D contiguous float32 GPU table of a group with weight_decay == 0 -- is stepped on
        the rows its backward MARKED only: allocates, once, a zero [E, d] gradient buffer and a zero row bitmap
        (`touched_rows(param)`).  A backward that knows the pair (kge_amd.model's score_spo / score_neg /
        score_neg_blocks nodes) accumulates the table's gradient into the buffer, marks the rows it adds to and leaves
        `param.grad` None; step() runs the dense update's arithmetic on the marked rows and zeroes the buffer's rows
        and the bitmap again.  With weight_decay == 0 a dense Adagrad step leaves a row whose gradient is zero bit for
        bit as it was, so this is the same optimizer without the passes over the whole table."""
        name = "kge_amd.optim.Adagrad.enable_touched_rows"
        group = next((g for g in self.param_groups if any(q is param for q in g["params"])), None)
        if group is None:
            raise ValueError(f"{name}: not a parameter of this optimizer")
        if not (torch.is_tensor(param) and param.is_cuda and param.dim() == 2 and param.dtype == torch.float32
                and param.is_contiguous()):
            raise ValueError(f"{name}: needs a 2-D contiguous float32 GPU parameter")
        if group["weight_decay"] != 0:
            raise ValueError(f"{name}: weight decay moves rows without a gradient: the group's weight_decay must be 0")
        if param not in self._touched:
            self._touched[param] = (torch.zeros_like(param, requires_grad=False).detach(),
                                    engine.touched_bitmap(param.shape[0], param.device))
        return self._touched[param]

    def touched_rows(self, param):
        """(grad, bitmap) of a parameter switched to the touched-row step, else None."""
        return self._touched.get(param)

    def stepped_params(self):
        """The parameters the last step() updated (kge_amd.train_graph.GraphedStep: `p.grad is not None` misses the
        touched-row parameters, whose gradient never reaches `.grad`)."""
        return list(self._stepped)

    def _step_touched(self, p, group, fold=False):
        if p.grad is not None:
            raise RuntimeError("kge_amd.optim.Adagrad: a dense gradient reached a parameter switched to the touched-row "
                               "step (a backward route that does not know its gradient buffer)")
        if p in self._penalties and p not in self._wpen:
            raise RuntimeError("kge_amd.optim.Adagrad: a fused penalty on a parameter switched to the touched-row step "
                               "(an unweighted term touches every row)")
        if group["weight_decay"] != 0:
            raise RuntimeError("kge_amd.optim.Adagrad: weight_decay was set on a group with a touched-row parameter")
        grad, bitmap = self._touched[p]
        state = self.state[p]
        state["step"] += 1
        step = float(state["step"])
        minus_clr = -float(group["lr"]) / (1.0 + (step - 1.0) * group["lr_decay"])
        copy = None
        if self.bf16_copies:
            # only the marked rows are rewritten: the copy must be FRESH before (as _step_rows)
            copy = bf16_copy_of(p)
            if copy is None:
                rec = getattr(p, BF16_ATTR, None)
                if rec is not None and rec[0].shape == p.shape and rec[0].data_ptr() != 0:
                    copy = rec[0]
                    copy.copy_(p.detach())
                else:
                    copy = p.detach().to(torch.bfloat16)
        if fold and p in self._wpen:
            engine.adagrad_step_touched_wpenalty(p.detach(), grad, state["sum"], bitmap, minus_clr, float(group["eps"]),
                                                 self._wpenalty_seg(p), copy)
        else:
            engine.adagrad_step_touched(p.detach(), grad, state["sum"], bitmap, minus_clr, float(group["eps"]), copy)
        torch.autograd.graph.increment_version(p)
        if copy is not None:
            setattr(p, BF16_ATTR, (copy, p._version, p.data_ptr()))

    @staticmethod
    def _aligned(*tensors) -> bool:
        """The dense kernels load and store four floats at a time: kge_adagrad_step* / kge_adam_step refuse a param,
        grad or state pointer that is not 16-byte aligned.  A contiguous view at an odd element offset of a flat
        buffer (nn.Parameter(flat[1:1 + k]), a gradient that is a slice of a flattened gradient buffer) is not."""
        return all(t.data_ptr() % 16 == 0 for t in tensors)

    @staticmethod
    def _kernel_ok(p: torch.Tensor) -> bool:
        g = p.grad
        return (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g is not None
                and not g.is_sparse and g.dtype == torch.float32 and g.is_contiguous() and Adagrad._aligned(p, g))

    @staticmethod
    def _rows_ok(p: torch.Tensor, group) -> bool:
        """Row-sparse gradient of a 2-D table (lookup_embedder.sparse: True -> nn.Embedding(sparse=True),
        lookup_embedder.py:44-46): kge_adagrad_step_rows touches only the rows that have a gradient."""
        g = p.grad
        return (g is not None and g.is_sparse and p.is_cuda and p.dim() == 2 and p.dtype == torch.float32
                and p.is_contiguous() and g.dtype == torch.float32 and group["weight_decay"] == 0)

    def _step_rows(self, p, group):
        state = self.state[p]
        state["step"] += 1
        step = float(state["step"])
        minus_clr = -float(group["lr"]) / (1.0 + (step - 1.0) * group["lr_decay"])
        g = p.grad.coalesce()  # unique row ids, summed value rows (what torch's sparse Adagrad does first)
        rows = g.indices()[0].contiguous()
        vals = g.values().contiguous()
        if rows.numel() == 0:
            return
        s = state["sum"]
        copy = None
        if self.bf16_copies:
            # only the touched rows are rewritten below: the copy must be FRESH before (a parameter changed behind
            # the optimizer's back -- load_state_dict into the same Parameter, a re-init, a dense torch step --
            # leaves every other row stale); a stale or missing one is re-cast once, into the old buffer if it fits
            copy = bf16_copy_of(p)
            if copy is None:
                rec = getattr(p, BF16_ATTR, None)
                if rec is not None and rec[0].shape == p.shape and rec[0].data_ptr() != 0:
                    copy = rec[0]
                    copy.copy_(p.detach())
                else:
                    copy = p.detach().to(torch.bfloat16)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().kge_adagrad_step_rows(
                p.data_ptr(), p.stride(0), vals.data_ptr(), vals.stride(0), s.data_ptr(), s.stride(0), rows.data_ptr(),
                rows.numel(), p.shape[1], minus_clr, float(group["eps"]), None if copy is None else copy.data_ptr(),
                0 if copy is None else copy.stride(0), engine._stream(p.device)), "kge_adagrad_step_rows")
        torch.autograd.graph.increment_version(p)
        if copy is not None:
            setattr(p, BF16_ATTR, (copy, p._version, p.data_ptr()))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dense = {}  # device -> [(p, copy, segment)]: every dense table of a device in ONE launch (kge_adagrad_step_multi)
        stepped = self._stepped = []
        # (with a weighted term on a touched-row parameter the accumulators must be clear before the first launch)
        fold_touched = self._begin_fold() if self._wpen and self._touched else False
        for group in self.param_groups:
            if group.get("maximize") or group.get("differentiable"):
                raise NotImplementedError("kge_amd.optim.Adagrad: maximize / differentiable are not supported")
            rest = []
            for p in group["params"]:
                if self._touched and p in self._touched:
                    self._step_touched(p, group, fold_touched)
                    stepped.append(p)
                    continue
                if p.grad is None:
                    continue
                stepped.append(p)
                if self._rows_ok(p, group):
                    self._step_rows(p, group)
                    continue
                if not self._kernel_ok(p) or not self._aligned(self.state[p]["sum"]):
                    rest.append(p)
                    continue
                state = self.state[p]
                state["step"] += 1
                step = float(state["step"])
                minus_clr = -float(group["lr"]) / (1.0 + (step - 1.0) * group["lr_decay"])
                s = state["sum"]
                copy = None
                if self.bf16_copies and p.dim() == 2:
                    rec = getattr(p, BF16_ATTR, None)
                    copy = rec[0] if rec is not None and rec[0].shape == p.shape else \
                        torch.empty(p.shape, dtype=torch.bfloat16, device=p.device)
                seg = _lib.KgeAdagradSeg(p.data_ptr(), p.grad.data_ptr(), s.data_ptr(),
                                         None if copy is None else copy.data_ptr(), p.numel(), minus_clr,
                                         float(group["weight_decay"]), float(group["eps"]))
                dense.setdefault(p.device, []).append((p, copy, seg))
            if rest:  # torch's own update for everything else
                if any(p in self._penalties for p in rest) and not self._pen_off_once:
                    raise RuntimeError("kge_amd.optim.Adagrad: a parameter with a fused penalty left the kernel path")
                grads = [p.grad for p in rest]
                sums = [self.state[p]["sum"] for p in rest]
                steps = [self.state[p]["step"] for p in rest]
                _functional_adagrad(rest, grads, sums, steps, has_sparse_grad=any(g.is_sparse for g in grads),
                                    foreach=False, lr=group["lr"], weight_decay=group["weight_decay"],
                                    lr_decay=group["lr_decay"], eps=group["eps"], maximize=False)
        if self._wpen and self._touched:
            with_pen, self._pen_off_once = fold_touched, False
        else:
            with_pen = self._fold_this_step()
        for device, items in dense.items():
            with torch.cuda.device(device):
                if with_pen and self._wpen:  # the tables with a weighted term: launches of their own
                    heavy = [c for c in items if c[0] in self._wpen]
                    for i in range(0, len(heavy), _lib.ADAGRAD_MAX_SEGS):
                        chunk = heavy[i:i + _lib.ADAGRAD_MAX_SEGS]
                        segs = (_lib.KgeAdagradSeg * len(chunk))(*(c[2] for c in chunk))
                        pens = (_lib.KgeWPenaltySeg * len(chunk))(*(self._wpenalty_seg(c[0]) for c in chunk))
                        _lib.check(_lib.lib().kge_adagrad_step_multi_wpenalty(segs, pens, len(chunk),
                                                                              engine._stream(device)),
                                   "kge_adagrad_step_multi_wpenalty")
                    items_here = [c for c in items if c[0] not in self._wpen]
                else:
                    items_here = items
                for i in range(0, len(items_here), _lib.ADAGRAD_MAX_SEGS):
                    chunk = items_here[i:i + _lib.ADAGRAD_MAX_SEGS]
                    segs = (_lib.KgeAdagradSeg * len(chunk))(*(c[2] for c in chunk))
                    pens = self._penalty_segs([c[0] for c in chunk], device) if with_pen else None
                    if pens is not None:
                        _lib.check(_lib.lib().kge_adagrad_step_multi_penalty(segs, pens, len(chunk),
                                                                             engine._stream(device)),
                                   "kge_adagrad_step_multi_penalty")
                        continue
                    _lib.check(_lib.lib().kge_adagrad_step_multi(segs, len(chunk), engine._stream(device)),
                               "kge_adagrad_step_multi")
            for p, copy, _seg in items:
                torch.autograd.graph.increment_version(p)  # the kernel wrote through the raw pointer
                if copy is not None:
                    setattr(p, BF16_ATTR, (copy, p._version, p.data_ptr()))
        return loss


class Adam(_FoldedPenalties, torch.optim.Adam):
    """torch.optim.Adam (same constructor arguments and `state_dict`: "step", "exp_avg", "exp_avg_sq")
    with the dense update of float32 GPU parameters done by kge_adam_step: one pass instead of the
    multi-tensor sequence, optionally writing the bf16 scoring copies in the same pass.  amsgrad,
    maximize, capturable and differentiable are not supported; parameters the kernel does not cover
    are stepped by torch's own Adam.

    device_step=True: the step count lives on the device too.  Every parameter gets a 32-byte clock record
    (state[p]["clock"]: t, beta1^t, beta2^t and the two bias-correction floats; include/kge_amd.h kge_adam_clock) that
    a small kernel advances in front of the update; step() computes nothing from the step count, updates every dense
    table of a device in one launch (kge_adam_step_multi) and can fold the embedders' penalty terms into it
    (set_penalty, as kge_amd.optim.Adagrad).  Such an instance is `graph_capturable`.  The record is seeded from the
    host's state["step"] (T = 0, or the step count a checkpoint restored) with beta ** T and is not part of
    `state_dict()`: the checkpoint format stays step / exp_avg / exp_avg_sq.  The record carries powers of the betas
    it was seeded with: change a group's betas only together with dropping state[p]["clock"]."""

    # step() computes lr / (1 - beta1^t) and sqrt(1 - beta2^t) on the host from the step count and hands them to the
    # kernel as launch arguments: a hipGraph capture would freeze them at the capture step.  GraphedStep refuses --
    # unless the instance keeps the step count on the device (device_step=True sets the instance's attribute).
    graph_capturable = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 bf16_copies: bool = False, device_step: bool = False, **kw):
        kw.pop("foreach", None)
        kw.pop("fused", None)
        if amsgrad:
            raise NotImplementedError("kge_amd.optim.Adam: amsgrad is not supported")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False,
                         **kw)
        self.bf16_copies = bool(bf16_copies)
        self.device_step = bool(device_step)
        self._init_penalties()
        if self.device_step:
            self.graph_capturable = True

    def set_penalty(self, param, kind, p, weight, times=1.0, weighted=False):
        if not self.device_step:
            raise ValueError("kge_amd.optim.Adam: fused penalties need device_step=True (kge_adam_step_multi)")
        super().set_penalty(param, kind, p, weight, times, weighted)

    def after_graph_replay(self, params):
        """`params`: the parameters the captured step() updated.  The replayed clock kernel advanced their device
        records; the host's state["step"] -- what the checkpoint carries and a record is seeded from -- follows."""
        for p in params:
            st = self.state.get(p)
            if st is not None and "step" in st:
                st["step"] += 1

    def device_step_count(self, param) -> int:
        """`t` of the parameter's device clock record (a host read: synchronizes)."""
        return int(self.state[param]["clock"][0])

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: {n: v for n, v in st.items() if n != "clock"} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            st.pop("clock", None)  # seeded again from the restored state["step"] by the next step()

    def _clock_of(self, p, state, beta1, beta2) -> torch.Tensor:
        clock = state.get("clock")
        if clock is None or clock.device != p.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("kge_amd.optim.Adam: the first step() of a parameter cannot be captured "
                                   "(its state and clock record are made on the host): take one step eagerly first")
            import struct
            t = int(state["step"])
            rec = struct.pack("<qddff", t, float(beta1) ** t, float(beta2) ** t, 0.0, 0.0)
            clock = state["clock"] = torch.frombuffer(bytearray(rec), dtype=torch.int64).to(p.device)
        return clock

    def _step_device(self):
        dense, held = {}, False  # device -> [(p, copy, segment)]: every dense table of a device in ONE launch
        for group in self.param_groups:
            if group.get("maximize") or group.get("differentiable") or group.get("capturable"):
                raise NotImplementedError("kge_amd.optim.Adam: maximize / differentiable / capturable are not supported")
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if not Adagrad._kernel_ok(p) or (len(state) != 0 and not Adagrad._aligned(state["exp_avg"],
                                                                                         state["exp_avg_sq"])):
                    if p in self._penalties and not self._pen_off_once:
                        raise RuntimeError("kge_amd.optim.Adam: a parameter with a fused penalty left the kernel path")
                    held = True
                    continue
                if len(state) == 0:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("kge_amd.optim.Adam: the first step() of a parameter cannot be captured "
                                           "(its moments would be zeroed by every replay): take one step eagerly first")
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                clock = self._clock_of(p, state, beta1, beta2)
                state["step"] += 1  # (the checkpoint's count; the kernel's own is the record's t)
                copy = None
                if self.bf16_copies and p.dim() == 2:
                    rec = getattr(p, BF16_ATTR, None)
                    copy = rec[0] if rec is not None and rec[0].shape == p.shape else \
                        torch.empty(p.shape, dtype=torch.bfloat16, device=p.device)
                seg = _lib.KgeAdamSeg(p.data_ptr(), p.grad.data_ptr(), state["exp_avg"].data_ptr(),
                                      state["exp_avg_sq"].data_ptr(), None if copy is None else copy.data_ptr(),
                                      clock.data_ptr(), p.numel(), float(group["lr"]), float(beta1), float(beta2),
                                      float(group["weight_decay"]), float(group["eps"]))
                dense.setdefault(p.device, []).append((p, copy, seg))
        with_pen = self._fold_this_step()
        for device, items in dense.items():
            with torch.cuda.device(device):
                if with_pen and self._wpen:  # the tables with a weighted term: launches of their own
                    heavy = [c for c in items if c[0] in self._wpen]
                    for i in range(0, len(heavy), _lib.ADAM_MAX_SEGS):
                        chunk = heavy[i:i + _lib.ADAM_MAX_SEGS]
                        segs = (_lib.KgeAdamSeg * len(chunk))(*(c[2] for c in chunk))
                        pens = (_lib.KgeWPenaltySeg * len(chunk))(*(self._wpenalty_seg(c[0]) for c in chunk))
                        _lib.check(_lib.lib().kge_adam_step_multi_wpenalty(segs, pens, len(chunk),
                                                                           engine._stream(device)),
                                   "kge_adam_step_multi_wpenalty")
                    items_here = [c for c in items if c[0] not in self._wpen]
                else:
                    items_here = items
                for i in range(0, len(items_here), _lib.ADAM_MAX_SEGS):
                    chunk = items_here[i:i + _lib.ADAM_MAX_SEGS]
                    segs = (_lib.KgeAdamSeg * len(chunk))(*(c[2] for c in chunk))
                    pens = self._penalty_segs([c[0] for c in chunk], device) if with_pen else None
                    _lib.check(_lib.lib().kge_adam_step_multi(segs, pens, len(chunk), engine._stream(device)),
                               "kge_adam_step_multi")
            for p, copy, _seg in items:
                torch.autograd.graph.increment_version(p)  # the kernel wrote through the raw pointer
                if copy is not None:
                    setattr(p, BF16_ATTR, (copy, p._version, p.data_ptr()))
        return [c[0] for items in dense.values() for c in items], held

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.device_step:
            done, held = self._step_device()
            if held:
                self._torch_step_of_the_rest(done)
            return loss
        done, held = [], False
        for group in self.param_groups:
            if group.get("maximize") or group.get("differentiable") or group.get("capturable"):
                raise NotImplementedError("kge_amd.optim.Adam: maximize / differentiable / capturable are not supported")
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if not Adagrad._kernel_ok(p) or (len(state) != 0 and not Adagrad._aligned(state["exp_avg"],
                                                                                         state["exp_avg_sq"])):
                    held = True
                    continue
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                t = float(state["step"])
                step_size = float(group["lr"]) / (1.0 - beta1 ** t)
                bc2_sqrt = (1.0 - beta2 ** t) ** 0.5
                copy = None
                if self.bf16_copies and p.dim() == 2:
                    rec = getattr(p, BF16_ATTR, None)
                    copy = rec[0] if rec is not None and rec[0].shape == p.shape else \
                        torch.empty(p.shape, dtype=torch.bfloat16, device=p.device)
                with torch.cuda.device(p.device):
                    _lib.check(_lib.lib().kge_adam_step(
                        p.data_ptr(), p.grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(),
                        p.numel(), step_size, bc2_sqrt, float(beta1), float(beta2), float(group["weight_decay"]),
                        float(group["eps"]), None if copy is None else copy.data_ptr(), engine._stream(p.device)),
                        "kge_adam_step")
                torch.autograd.graph.increment_version(p)
                if copy is not None:
                    setattr(p, BF16_ATTR, (copy, p._version, p.data_ptr()))
                done.append(p)
        if held:
            self._torch_step_of_the_rest(done)
        return loss

    def _torch_step_of_the_rest(self, done):
        """torch's own update for everything else: hide the stepped parameters' gradients for the call."""
        stash = [(q, q.grad) for q in done]
        for q, _ in stash:
            q.grad = None
        try:
            torch.optim.Adam.step(self)
        finally:
            for q, g in stash:
                q.grad = g


class _TouchedRows(tuple):
    """(grad, bitmap) of SparseAdam.enable_touched_rows.  `pending`: a backward accumulated into the pair since the last
    step() -- set by the backward nodes of kge_amd.model; what `p.grad is not None` tells torch.optim.SparseAdam."""
    pending = False


class SparseAdam(_FoldedPenalties, torch.optim.SparseAdam):
    """torch.optim.SparseAdam (same constructor arguments and `state_dict`: "step", "exp_avg", "exp_avg_sq"; a
    checkpoint of either class loads into the other) for tables whose backward marks the rows it touched
    (`enable_touched_rows`, as kge_amd.optim.Adagrad): kge_sparse_adam_step_touched applies torch's row-wise update to
    the marked rows, with the step count on the device (state[p]["clock"], a kge_adam_clock record as
    Adam(device_step=True) keeps, not part of `state_dict()`), so the step is `graph_capturable`.
    Parameters that arrive with a genuinely sparse gradient are stepped by torch's own code; a dense gradient raises
    torch's error: SparseAdam has no dense form -- a dense Adam step moves rows that have no gradient."""

    graph_capturable = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, maximize=False, weight_decay=0,
                 bf16_copies: bool = False):
        if weight_decay != 0:
            raise ValueError("kge_amd.optim.SparseAdam: weight_decay moves rows without a gradient: it must be 0")
        if maximize:
            raise NotImplementedError("kge_amd.optim.SparseAdam: maximize is not supported")
        super().__init__(params, lr=lr, betas=betas, eps=eps, maximize=False)
        self.bf16_copies = bool(bf16_copies)
        self._touched = {}   # parameter -> _TouchedRows(persistent dense gradient [rows, d], bitmap)
        self._stepped = []   # the parameters the last step() updated: stepped_params
        self._init_penalties()

    def set_penalty(self, param, kind, p, weight, times=1.0, weighted=False):
        """A WEIGHTED penalty term on a touched-row parameter inside the row update (kge_amd.optim.Adagrad.set_penalty
        describes the arguments; kge_sparse_adam_step_touched_wpenalty).  An unweighted term touches every row:
        SparseAdam has no step for it."""
        if kind is not None and not weighted:
            raise ValueError("kge_amd.optim.SparseAdam: an unweighted penalty touches every row; only weighted=True "
                             "has a kernel")
        if kind is not None and param not in self._touched:
            raise ValueError("kge_amd.optim.SparseAdam: fused penalties are for touched-row parameters "
                             "(enable_touched_rows first)")
        super().set_penalty(param, kind, p, weight, times, weighted)

    def enable_touched_rows(self, param):
        """From now on `param` -- a 2-D contiguous float32 GPU table -- is stepped on the rows its backward MARKED:
        allocates, once, a zero [rows, d] gradient buffer and a zero row bitmap (`touched_rows(param)`).  A backward
        that knows the pair (kge_amd.model's score_spo / score_neg / score_neg_blocks nodes) accumulates the table's
        gradient into the buffer, marks the rows it adds to, sets the pair's `pending` and leaves `param.grad` None;
        step() applies torch.optim.SparseAdam's update to the marked rows -- the index set of the coalesced sparse
        gradient `sparse=True` embeddings would have produced -- and zeroes the buffer's rows and the bitmap again."""
        name = "kge_amd.optim.SparseAdam.enable_touched_rows"
        group = next((g for g in self.param_groups if any(q is param for q in g["params"])), None)
        if group is None:
            raise ValueError(f"{name}: not a parameter of this optimizer")
        if not (torch.is_tensor(param) and param.is_cuda and param.dim() == 2 and param.dtype == torch.float32
                and param.is_contiguous()):
            raise ValueError(f"{name}: needs a 2-D contiguous float32 GPU parameter")
        if param not in self._touched:
            self._touched[param] = _TouchedRows((torch.zeros_like(param, requires_grad=False).detach(),
                                                 engine.touched_bitmap(param.shape[0], param.device)))
        return self._touched[param]

    def touched_rows(self, param):
        """(grad, bitmap) of a parameter switched to the touched-row step, else None."""
        return self._touched.get(param)

    def stepped_params(self):
        """The parameters the last step() updated (kge_amd.train_graph.GraphedStep: `p.grad is not None` misses the
        touched-row parameters, whose gradient never reaches `.grad`)."""
        return list(self._stepped)

    def after_graph_replay(self, params):
        """`params`: the parameters the captured step() updated.  The replayed clock kernel advanced their device
        records; the host's state["step"] -- what the checkpoint carries and a record is seeded from -- follows."""
        for p in params:
            st = self.state.get(p)
            if st is not None and "step" in st:
                st["step"] += 1

    def device_step_count(self, param) -> int:
        """`t` of the parameter's device clock record (a host read: synchronizes)."""
        return int(self.state[param]["clock"][0])

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: {n: v for n, v in st.items() if n != "clock"} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            st.pop("clock", None)  # seeded again from the restored state["step"] by the next step()

    def _step_touched(self, p, group, fold=False):
        name = "kge_amd.optim.SparseAdam"
        if p.grad is not None:
            raise RuntimeError(f"{name}: a gradient reached `.grad` of a parameter switched to the touched-row step (a "
                               "backward route that does not know its gradient buffer)")
        pair = self._touched[p]
        if not pair.pending:  # no backward touched the table: torch skips a parameter whose grad is None
            return False
        capturing = torch.cuda.is_current_stream_capturing()
        state = self.state[p]
        if len(state) == 0:
            if capturing:
                raise RuntimeError(f"{name}: the first step() of a parameter cannot be captured (its moments would be "
                                   "zeroed by every replay): take one step eagerly first")
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        beta1, beta2 = group["betas"]
        clock = state.get("clock")
        if clock is None or clock.device != p.device:
            if capturing:
                raise RuntimeError(f"{name}: the first step() of a parameter cannot be captured (its clock record is "
                                   "made on the host): take one step eagerly first")
            import struct
            t = int(state["step"])
            rec = struct.pack("<qddff", t, float(beta1) ** t, float(beta2) ** t, 0.0, 0.0)
            clock = state["clock"] = torch.frombuffer(bytearray(rec), dtype=torch.int64).to(p.device)
        state["step"] += 1  # (the checkpoint's count; the kernel's own is the record's t)
        pair.pending = False
        grad, bitmap = pair
        copy = None
        if self.bf16_copies:
            # only the marked rows are rewritten: the copy must be FRESH before (as Adagrad._step_touched)
            copy = bf16_copy_of(p)
            if copy is None:
                rec = getattr(p, BF16_ATTR, None)
                if rec is not None and rec[0].shape == p.shape and rec[0].data_ptr() != 0:
                    copy = rec[0]
                    copy.copy_(p.detach())
                else:
                    copy = p.detach().to(torch.bfloat16)
        if fold and p in self._wpen:
            engine.sparse_adam_step_touched_wpenalty(p.detach(), grad, state["exp_avg"], state["exp_avg_sq"], bitmap,
                                                     clock, float(group["lr"]), float(beta1), float(beta2),
                                                     float(group["eps"]), self._wpenalty_seg(p), copy)
        else:
            engine.sparse_adam_step_touched(p.detach(), grad, state["exp_avg"], state["exp_avg_sq"], bitmap, clock,
                                            float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), copy)
        torch.autograd.graph.increment_version(p)
        if copy is not None:
            setattr(p, BF16_ATTR, (copy, p._version, p.data_ptr()))
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group.get("maximize"):
                raise NotImplementedError("kge_amd.optim.SparseAdam: maximize is not supported")
        # torch's own step first: the parameters with a sparse gradient; its error for a dense one.  (The touched-row
        # parameters have no `.grad`: it skips them.)
        stepped = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        for p in stepped:
            if self._touched and p in self._touched:
                self._step_touched(p, None)  # raises: a gradient in `.grad`
        torch.optim.SparseAdam.step(self)
        if self._touched:
            fold = self._fold_this_step() if self._penalties else False
            for group in self.param_groups:
                for p in group["params"]:
                    if p in self._touched and self._step_touched(p, group, fold):
                        stepped.append(p)
        self._stepped = stepped
        return loss
