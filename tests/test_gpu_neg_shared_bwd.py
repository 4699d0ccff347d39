"""kge_score_neg_shared_bwd_accum -- sns_fold_base_kernel, sns_fold_repeat_kernel and both roles of
neg_shared_bwd_kernel (score_neg_shared.hip) -- on float32 tables against the float64 reference of
tests/_neg_shared_bwd_ref.py (_neg_bwd_ref.neg_bwd_accum on the materialised samples), inside the derived rounding bound
(K_e + C) u A_e of that module: elementwise, on grad_ent and grad_rel, both slots, naive and default sampling.

The entry is called through ctypes on raw pointers, so that pitches, index types and the workspace are the test's own.
grad_ent and grad_rel sit inside one NaN-bit-filled arena with 4 KiB before, between and behind them (test_gpu_neg_bwd's
_Arena); every float outside the [rows, dim] windows must keep its bits, the pitch columns included.  The workspace is
exactly kge_score_neg_shared_workspace_bytes long and NaN-filled, inside a larger NaN-filled allocation whose
surroundings must keep their bits.  A fixed case list, each shape chosen for a branch of the launch rules (DESIGN.md,
"Shared-negative backward against float64"); tests/test_neg_shared_bwd_ref_cpu.py holds the reference to float64
autograd and to its folded second statement, asserts the branch of every case and shows, on these very inputs, that the
planted defects exceed the bound 8 times over.  No tolerance in this file is measured.

Every case prints its largest err / bound per table (profiles/neg_shared_bwd_bound.txt is one such run)."""
import ctypes

import numpy as np
import pytest
import torch

import _neg_bwd_ref as NB
import _neg_shared_bwd_ref as S
from test_gpu_neg_bwd import DEV, NAN_BITS, PAD, _Arena, _grad_arena, _ix, _ptr, _t

pytestmark = pytest.mark.gpu
INVALID_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -5


def _distance(k):
    return k["name"] in ("transe", "rotate") and k["l_norm"] != 1.0


def _device(k, bf16=False):
    """tables, index operands, the shared sample, gout and scores on the device, on the pitches and index types of the
    case"""
    from kge_amd import engine as eng
    n, d, E, K, pitched = k["n"], k["d"], k["E"], k["K"], bool(k.get("pitched"))
    ent, rel = _t(k["ent"]), _t(k["rel"])
    if pitched:  # the entity table on a row pitch
        buf = torch.full((E, d + 4), float("nan"), device=DEV)
        buf[:, :d] = ent
        ent = buf[:, :d]
    if bf16:
        ent, rel = ent.bfloat16(), rel.bfloat16()
    T = eng.Tables(k["name"], ent, rel, l_norm=k["l_norm"])
    s, p, o = _t(k["s"]), _t(k["p"]), _t(k["o"])
    if pitched:  # int32 columns of one [n, 3] triple tensor: stride 3
        tr = torch.stack([s, p, o], dim=1).to(torch.int32).contiguous()
        s, p, o = tr[:, 0], tr[:, 1], tr[:, 2]
    unique = _t(k["unique"])
    if pitched or k["slot"] == 2:
        unique = unique.to(torch.int32)
    drop = None if k["drop"] is None else _t(k["drop"])
    repeat = _t(k["repeat"])
    gout = _t(k["gout"])
    if pitched:  # a slice of a wider NaN-filled matrix
        gw = torch.full((n, K + 3), float("nan"), device=DEV)
        gw[:, 1:1 + K] = gout
        gout = gw[:, 1:1 + K]
    scores = None
    if _distance(k) and not bf16:  # the forward's float32 scores: the distance comes from them
        scores = eng.score_neg_shared(T, s, p, o, k["slot"], unique, drop, repeat)
        if pitched:
            wide = torch.full((n, K + 6), float("nan"), device=DEV)
            wide[:, 3:3 + K] = scores
            scores = wide[:, 3:3 + K]
    return dict(T=T, s=s, p=p, o=o, unique=unique, drop=drop, repeat=repeat, gout=gout, scores=scores)


class _Workspace:
    """`nbytes` of NaN-filled scratch inside a larger NaN-filled allocation"""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.nbytes, self.n = nbytes, nbytes // 4
        self.buf = torch.full((2 * PAD + self.n,), float("nan"), device=DEV)
        assert self.ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def surroundings_intact(self):
        bits = self.buf.view(torch.int32)
        return bool((bits[:PAD] == NAN_BITS).all()) and bool((bits[PAD + self.n:] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == NAN_BITS).all())


def _workspace(k, dev):
    from kge_amd import _lib
    tc = dev["T"].c()
    need = _lib.lib().kge_score_neg_shared_workspace_bytes(ctypes.byref(tc), k["n"], k["Uc"])
    assert need > 0 and need % 256 == 0
    return _Workspace(need)


def _call(k, dev, ar, ws, scores="own", n=None, uc=None, nrep=None, ws_bytes=None):
    """kge_score_neg_shared_bwd_accum through ctypes on the arena's and the workspace's pointers -> return code"""
    from kge_amd import _lib
    from kge_amd import engine as eng
    (si, pi, oi), keep = _ix(dev)
    tc = dev["T"].c()
    sc = dev["scores"] if scores == "own" else scores
    gout, uq, rep = dev["gout"], dev["unique"], dev["repeat"]
    n = k["n"] if n is None else n
    uc = k["Uc"] if uc is None else uc
    nrep = rep.numel() if nrep is None else nrep
    row = lambda x: x.stride(0) if x.shape[0] > 1 else max(k["K"], 1)
    return _lib.lib().kge_score_neg_shared_bwd_accum(
        ctypes.byref(tc), si, pi, oi, n, k["slot"], uq.data_ptr(), _lib.I32 if uq.dtype == torch.int32 else _lib.I64, uc,
        _ptr(dev["drop"]), rep.data_ptr() if nrep else None, nrep, gout.data_ptr(), row(gout), _ptr(sc),
        0 if sc is None else row(sc), ar.ptr(0), ar.shapes[0][2], ar.ptr(1), ar.shapes[1][2], ws.ptr(),
        ws.nbytes if ws_bytes is None else ws_bytes, eng._stream_handle(DEV))


def _compare(label, got, want, bound, names=("grad_ent", "grad_rel")):
    worst = []
    for g, w, b in zip(got, want, bound):
        assert np.isfinite(g).all(), label
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / b, 0.0)
        worst.append(float(r.max()) if r.size else 0.0)
    print(f"neg_shared_bwd {label}: max err / bound  " + "  ".join(f"{nm} {x:.4f}" for nm, x in zip(names, worst)))
    for g, w, b, nm in zip(got, want, bound, names):
        bad = np.abs(g - w) > b  # (an element no occurrence goes to: bound 0, equal as a number)
        assert not bad.any(), (label, nm, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)


def _check(label, ar, ws, want, bound):
    assert ar.guards_intact(), label
    assert ws is None or ws.surroundings_intact(), label
    _compare(label, [ar.get(0), ar.get(1)], want, bound)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_shared_bwd_within_bound(case):
    for slot in (0, 2):
        k = S.make_case(case, slot)
        want, bound = NB.reference(k)
        dev = _device(k)
        ar = _grad_arena(k, k["rel"].shape[1])
        ws = _workspace(k, dev)
        label = f"{S.case_id(case)} slot {slot}"
        if _distance(k):
            before = ar.buf.view(torch.int32).clone()
            assert _call(k, dev, ar, ws, scores=None) == INVALID_ARG
            torch.cuda.synchronize()
            assert torch.equal(ar.buf.view(torch.int32), before) and ws.untouched(), label
        assert _call(k, dev, ar, ws) == 0
        torch.cuda.synchronize()
        _check(label, ar, ws, want, bound)


def test_status_codes_leave_gradients_and_workspace_alone():
    """scores == NULL with l_norm 2: KGE_ERR_INVALID_ARG; a workspace one byte short: KGE_ERR_WORKSPACE; bf16 tables,
    d = 1026 and d = 1025: KGE_ERR_UNSUPPORTED; n = 0 and Uc + repeats = 0: KGE_OK.  The NaN-bit-filled gradient buffers
    and the workspace keep their bits in every one."""
    from kge_amd import _lib
    assert (_lib.KGE_ERR_UNSUPPORTED, _lib.KGE_OK) == (UNSUPPORTED, 0)
    l2 = S._c("transe", 2, 5, 7, 33, "default", per=1, nrep=2)
    cx = S._c("complex", 1, 5, 7, 8, "default", nrep=2)
    nv = S._c("rotate", 1, 5, 7, 8, "naive", nrep=0)
    todo = [(l2, INVALID_ARG, dict(scores=None), False), (S._c("rotate", 2, 5, 7, 66, "naive", per=1), INVALID_ARG,
                                                          dict(scores=None), False),
            (cx, WORKSPACE, dict(short=1), False), (l2, WORKSPACE, dict(short=1), False),
            (cx, UNSUPPORTED, {}, True), (l2, UNSUPPORTED, {}, True),
            (S.UNSUPPORTED[0], UNSUPPORTED, {}, False), (S.UNSUPPORTED[1], UNSUPPORTED, {}, False),
            (cx, 0, dict(n=0), False), (nv, 0, dict(uc=0, nrep=0), False)]
    for case, rc, how, bf16 in todo:
        for slot in (0, 2):
            k = S.make_case(case, slot, seed=5)
            dev = _device(k, bf16)
            if bf16 and _distance(k):
                dev["scores"] = torch.zeros(k["n"], k["K"], device=DEV)
            dr = k["rel"].shape[1]
            ar = _Arena([(k["E"], k["d"], k["d"]), (k["R"], dr, dr)])
            ws = _workspace(k, dev)
            kw = {x: how[x] for x in how if x != "short"}
            if "short" in how:
                kw["ws_bytes"] = ws.nbytes - how["short"]
            got = _call(k, dev, ar, ws, **kw)
            torch.cuda.synchronize()
            assert got == rc, (S.case_id(case), slot, how, bf16, got)
            assert bool((ar.buf.view(torch.int32) == NAN_BITS).all()) and ws.untouched(), (S.case_id(case), slot, how)


def _first(pred):
    return next(c for c in S.CASES if pred(c))


ENGINE_CASES = [_first(lambda c, nc=nc: S.shared_nc(c["d"]) == nc and c["samp"] == "default" and c["n"] > 1)
                for nc in (1, 2, 4, 8)] + [_first(lambda c: c["l_norm"] == 2.0 and c["d"] == 130)]


@pytest.mark.parametrize("case", ENGINE_CASES, ids=S.case_id)
def test_engine_wrapper_within_bound(case):
    """engine.score_neg_shared_bwd_accum once per nc (and once with `scores`), on the same inputs and bound"""
    from kge_amd import engine as eng
    assert [S.shared_nc(c["d"]) for c in ENGINE_CASES] == [1, 2, 4, 8, 2]
    for slot in (0, 2):
        k = S.make_case(case, slot)
        want, bound = NB.reference(k)
        dev = _device(k)
        ar = _grad_arena(k, k["rel"].shape[1])
        assert eng.score_neg_shared_bwd_accum(dev["T"], dev["s"], dev["p"], dev["o"], slot, dev["unique"], dev["drop"],
                                              dev["repeat"], dev["gout"], dev["scores"], ar.window(0),
                                              ar.window(1)) is True
        torch.cuda.synchronize()
        _check(f"{S.case_id(case)} slot {slot} engine", ar, None, want, bound)


MODEL_CASES = [_first(lambda c, name=name: c["name"] == name and c["n"] >= 15 and c["samp"] == "default")
               for name in S.NAMES]


@pytest.mark.parametrize("case", MODEL_CASES, ids=S.case_id)
def test_model_backward_within_bound(case):
    """model.score_neg_shared(...).backward(gout) once per scorer: the table gradients inside the same bound"""
    from kge_amd import model
    for slot in (0, 2):
        k = S.make_case(case, slot)
        assert not k["preloaded"]
        want, bound = NB.reference(k)
        m = model.create(k["name"], k["E"], k["R"], k["d"], l_norm=k["l_norm"], device=DEV).train()
        we, wr = m.get_s_embedder().weight, m.get_p_embedder().weight
        assert we.shape == k["ent"].shape and wr.shape == k["rel"].shape
        with torch.no_grad():
            we.copy_(_t(k["ent"]))
            wr.copy_(_t(k["rel"]))
        got = m.score_neg_shared(_t(k["s"]), _t(k["p"]), _t(k["o"]), slot, _t(k["unique"]),
                                 None if k["drop"] is None else _t(k["drop"]), _t(k["repeat"]))
        assert got.shape == (k["n"], k["K"])
        got.backward(_t(k["gout"]))
        torch.cuda.synchronize()
        _compare(f"{S.case_id(case)} slot {slot} model", [we.grad.double().cpu().numpy(), wr.grad.double().cpu().numpy()],
                 want, bound)
