"""The triple-wise backward entry points of bwd.hip -- kge_score_spo_bwd, kge_score_spo_bwd_accum,
kge_score_neg_bwd_accum, kge_neg_order, kge_score_neg_bwd_accum_sorted -- on float32 tables against the float64 closed
forms of tests/_neg_bwd_ref.py, inside the derived rounding bound (K_e + C) u A_e of that module: elementwise, on
grad_ent and grad_rel, both slots, the atomic and the sorted entry on every neg case.

The entries are called through ctypes on raw pointers, so that pitches, rel_scratch == NULL and `order` are the test's
own.  Every gradient table sits inside one NaN-bit-filled arena with padding before, between and behind the tables;
every float outside the [rows, dim] windows must keep its bits (the pitch columns included).  A fixed case list, each
shape chosen for a branch of the launch rules ("Triple-wise backward against float64");
tests/test_neg_bwd_ref_cpu.py holds the reference to float64 autograd, asserts the branch of every case and shows, on
these very inputs, that the planted defects exceed the bound 8 times over.  No tolerance in this file is measured.

Every case prints its largest err / bound per output (profiles/neg_bwd_bound.txt is one such run)."""
import ctypes

import numpy as np
import pytest
import torch

import _neg_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 1024  # floats of NaN in front of, between and behind the gradient tables (tables stay 16-byte aligned)
NAN_BITS = 0x7FC00000
INVALID_ARG, UNSUPPORTED = -1, -2


def _t(x, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(DEV) if dtype is None else x.to(DEV, dtype)


class _Arena:
    """Tables of [rows, dim] floats on pitch `ld` inside ONE NaN-filled allocation"""

    def __init__(self, shapes):
        self.shapes, self.offs, off = shapes, [], PAD
        for rows, dim, ld in shapes:
            self.offs.append(off)
            off += (rows * ld + 3) // 4 * 4 + PAD
        self.buf = torch.full((off,), float("nan"), device=DEV)
        assert bool((self.buf.view(torch.int32) == NAN_BITS).all())

    def window(self, i, buf=None):
        rows, dim, ld = self.shapes[i]
        buf = self.buf if buf is None else buf
        return buf[self.offs[i]:self.offs[i] + rows * ld].view(rows, ld)[:, :dim]

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * self.offs[i]

    def load(self, arrays):
        for i, a in enumerate(arrays):
            self.window(i).copy_(_t(a))

    def guards_intact(self):
        """every float outside the windows still carries the NaN's bits"""
        bits = self.buf.view(torch.int32).clone()
        for i in range(len(self.shapes)):
            self.window(i, bits).fill_(NAN_BITS)
        return bool((bits == NAN_BITS).all())

    def get(self, i):
        return self.window(i).double().cpu().numpy()


def _device(k):
    """tables, index operands, neg, gout on the device, on the pitches and index types of the case"""
    from kge_amd import engine as eng
    n, d, E, pitched = k["n"], k["d"], k["E"], bool(k.get("pitched"))
    ent = _t(k["ent"])
    if pitched:  # the entity table on a row pitch
        buf = torch.full((E, d + 4), float("nan"), device=DEV)
        buf[:, :d] = ent
        ent = buf[:, :d]
    T = eng.Tables(k["name"], ent, _t(k["rel"]), l_norm=k["l_norm"])
    s, p, o = _t(k["s"]), _t(k["p"]), _t(k["o"])
    if pitched:  # int32 columns of one [n, 3] triple tensor: stride 3
        tr = torch.stack([s, p, o], dim=1).to(torch.int32).contiguous()
        s, p, o = tr[:, 0], tr[:, 1], tr[:, 2]
    dev = dict(T=T, s=s, p=p, o=o)
    cols = k["K"] if k["kind"] == "neg" else None
    gout = _t(k["gout"])
    if k["kind"] == "neg":
        neg = _t(k["neg"])
        if pitched:  # a column slice of a wider int32 matrix, gout a slice of a NaN-filled one
            wide = torch.zeros((n, cols + 5), dtype=torch.int32, device=DEV)  # (entity 0 around the slice: a low row)
            wide[:, 2:2 + cols] = neg.to(torch.int32)
            neg = wide[:, 2:2 + cols]
            gw = torch.full((n, cols + 3), float("nan"), device=DEV)
            gw[:, 1:1 + cols] = gout
            gout = gw[:, 1:1 + cols]
        elif k["slot"] == 2:
            neg = neg.to(torch.int32)
        dev.update(neg=neg)
    dev.update(gout=gout, scores=_scores(k, dev))
    return dev


def _scores(k, dev):
    """the forward's float32 scores: the distance models with l_norm != 1 take the distance from them"""
    from kge_amd import engine as eng
    if k["name"] in ("complex", "distmult") or k["l_norm"] == 1.0:
        return None
    if k["kind"] != "neg":
        return eng.score_spo(dev["T"], dev["s"], dev["p"], dev["o"])
    sc = eng.score_neg(dev["T"], dev["s"], dev["p"], dev["o"], k["slot"], dev["neg"])
    if k.get("pitched"):
        wide = torch.full((k["n"], k["K"] + 6), float("nan"), device=DEV)
        wide[:, 3:3 + k["K"]] = sc
        sc = wide[:, 3:3 + k["K"]]
    return sc


def _grad_arena(k, dr):
    """grad_ent and grad_rel of a case inside one arena (wider pitches where the case is pitched), pre-loaded"""
    extra = (5, 3) if k.get("pitched") else (0, 0)
    ar = _Arena([(k["E"], k["d"], k["d"] + extra[0]), (k["R"], dr, dr + extra[1])])
    ar.load([k["ge0"], k["gr0"]])
    return ar


def _ix(dev):
    from kge_amd import engine as eng
    keep = []
    return [eng._index(dev[x], DEV, keep) for x in "spo"], keep


def _ptr(x):
    return None if x is None else x.data_ptr()


def _neg_args(k, dev):
    from kge_amd import _lib
    neg = dev["neg"]
    return (k["n"], k["slot"], neg.data_ptr(), _lib.I32 if neg.dtype == torch.int32 else _lib.I64, neg.stride(0), k["K"])


def _neg_order(k, dev):
    """`order` of kge_score_neg_bwd_accum_sorted: histogram, exclusive prefix sums (torch), scatter -> (order, counts,
    cursor as the scatter left it)"""
    from kge_amd import _lib
    from kge_amd import engine as eng
    n, _, nptr, it, nld, K = _neg_args(k, dev)
    counts = torch.zeros(k["E"], dtype=torch.int64, device=DEV)
    order = torch.full((max(n * K, 1),), -1, dtype=torch.int64, device=DEV)
    st = eng._stream_handle(DEV)
    assert _lib.lib().kge_neg_order(nptr, it, nld, n, K, k["E"], counts.data_ptr(), None, st) == 0
    cursor = torch.cumsum(counts, 0).sub_(counts)
    assert _lib.lib().kge_neg_order(nptr, it, nld, n, K, k["E"], cursor.data_ptr(), order.data_ptr(), st) == 0
    return order[:n * K], counts, cursor


def _call_neg(k, dev, ar, entry, order=None, rot=None, scores="own"):
    """kge_score_neg_bwd_accum (entry "atomic") or _sorted through ctypes on the arena's pointers -> return code"""
    from kge_amd import _lib
    from kge_amd import engine as eng
    (si, pi, oi), keep = _ix(dev)
    tc = dev["T"].c()
    sc = dev["scores"] if scores == "own" else scores
    gout = dev["gout"]
    head = (ctypes.byref(tc), si, pi, oi) + _neg_args(k, dev)
    tail = (gout.data_ptr(), gout.stride(0), _ptr(sc), 0 if sc is None else sc.stride(0), ar.ptr(0), ar.shapes[0][2],
            ar.ptr(1), ar.shapes[1][2])
    st = eng._stream_handle(DEV)
    if entry == "atomic":
        return _lib.lib().kge_score_neg_bwd_accum(*head, *tail, st)
    return _lib.lib().kge_score_neg_bwd_accum_sorted(*head, order.data_ptr(), *tail, _ptr(rot), st)


def _check(label, ar, want, bound, names=("grad_ent", "grad_rel")):
    got = [ar.get(i) for i in range(len(want))]
    worst = []
    for g, w, b in zip(got, want, bound):
        assert np.isfinite(g).all(), label
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / b, 0.0)
        worst.append(float(r.max()) if r.size else 0.0)
    print(f"neg_bwd {label}: max err / bound  " + "  ".join(f"{nm} {x:.4f}" for nm, x in zip(names, worst)))
    assert ar.guards_intact(), label
    for g, w, b, nm in zip(got, want, bound, names):
        bad = np.abs(g - w) > b
        assert not bad.any(), (label, nm, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)


@pytest.mark.parametrize("case", R.NEG_CASES, ids=R.case_id)
def test_neg_bwd_within_bound(case):
    """both slots, the atomic and the sorted entry (RotatE: with rel_scratch and with NULL), each inside the same bound"""
    for slot in (0, 2):
        k = R.make_case(case, slot)
        want, bound = R.reference(k)
        dev = _device(k)
        dr = k["rel"].shape[1]
        order, _, _ = _neg_order(k, dev)
        runs = [("atomic", None)] + [("sorted", None)] + ([("sorted+scratch", True)] if k["name"] == "rotate" else [])
        for entry, scratch in runs:
            ar = _grad_arena(k, dr)
            rot = torch.full((k["R"], 2 * dr), float("nan"), device=DEV) if scratch else None
            assert _call_neg(k, dev, ar, "atomic" if entry == "atomic" else "sorted", order, rot) == 0
            torch.cuda.synchronize()
            _check(f"{R.case_id(case)} slot {slot} {entry}", ar, want, bound)


def test_neg_bwd_unsupported_and_invalid_leave_the_gradients_alone():
    """d = 1026: both entries return KGE_ERR_UNSUPPORTED; TransE / RotatE with l_norm != 1 and scores == NULL:
    KGE_ERR_INVALID_ARG; n = 0 and K = 0: KGE_OK.  In every case the NaN-bit-filled gradient buffers keep their bits."""
    from kge_amd import _lib
    assert (_lib.KGE_ERR_UNSUPPORTED, _lib.KGE_OK) == (UNSUPPORTED, 0)
    todo = [(R.NEG_UNSUPPORTED, UNSUPPORTED, {}),
            (R._neg("transe", 2, 5, 9, 33, 60), INVALID_ARG, dict(scores=None)),
            (R._neg("rotate", 3, 5, 9, 66, 60), INVALID_ARG, dict(scores=None)),
            (R._neg("complex", 1, 5, 9, 8, 60), 0, dict(n=0)), (R._neg("rotate", 1, 5, 9, 8, 60), 0, dict(K=0))]
    for case, rc, how in todo:
        for slot in (0, 2):
            k = R.make_case(case, slot, seed=5)
            dev = _device(k)
            order = torch.arange(k["n"] * k["K"], dtype=torch.int64, device=DEV)
            k.update({x: how[x] for x in how if x in ("n", "K")})  # (the operands keep their sizes: only the counts go)
            for entry in ("atomic", "sorted"):
                ar = _Arena([(k["E"], k["d"], k["d"]), (k["R"], k["rel"].shape[1], k["rel"].shape[1])])
                rot = torch.empty(k["R"], 2 * k["rel"].shape[1], device=DEV) if k["name"] == "rotate" else None
                got = _call_neg(k, dev, ar, entry, order, rot, **{x: how[x] for x in how if x == "scores"})
                torch.cuda.synchronize()
                assert got == rc, (R.case_id(case), slot, entry, got)
                assert bool((ar.buf.view(torch.int32) == NAN_BITS).all()), (R.case_id(case), slot, entry)


WRAPPER_CASES = [c for c in R.NEG_CASES if (c["n"], c["K"]) == (19, 70) and c["name"] in ("complex", "rotate")
                 and not c.get("pitched")]


@pytest.mark.parametrize("sorted_", [False, True], ids=["atomic", "sorted"])
def test_engine_wrapper_reaches_both_entries(sorted_, monkeypatch):
    """engine.score_neg_bwd_accum with NEG_BWD_SORTED forced either way: inside the same bound"""
    from kge_amd import engine as eng
    assert len(WRAPPER_CASES) == 2
    monkeypatch.setattr(eng, "NEG_BWD_SORTED", sorted_)
    for case in WRAPPER_CASES:
        for slot in (0, 2):
            k = R.make_case(case, slot)
            want, bound = R.reference(k)
            dev = _device(k)
            ar = _grad_arena(k, k["rel"].shape[1])
            assert eng.score_neg_bwd_accum(dev["T"], dev["s"], dev["p"], dev["o"], slot, dev["neg"], dev["gout"],
                                           dev["scores"], ar.window(0), ar.window(1)) is True
            torch.cuda.synchronize()
            _check(f"{R.case_id(case)} slot {slot} engine {'sorted' if sorted_ else 'atomic'}", ar, want, bound)


ORDER_CASES = [c for c in R.NEG_CASES if (c["name"], c["n"], c["K"]) in
               (("distmult", 1, 1), ("complex", 19, 70), ("complex", 450, 130), ("complex", 37, 131), ("distmult", 3, 11))]


@pytest.mark.parametrize("case", ORDER_CASES, ids=R.case_id)
def test_neg_order_is_an_exact_counting_sort(case):
    """kge_neg_order, exact integer results: the histogram is bincount; `order` is a permutation of 0 .. n K - 1 along
    which the ids do not decrease; entity e's positions fill [excl[e], excl[e + 1]); the clobbered cursor holds the
    inclusive sums -- int64 (slot 0), int32 (slot 2) and int32 on neg_ld > K (the pitched case)."""
    assert len(ORDER_CASES) == 6
    for slot in (0, 2):
        k = R.make_case(case, slot)
        dev = _device(k)
        order, counts, cursor = _neg_order(k, dev)
        torch.cuda.synchronize()
        flat = k["neg"].reshape(-1)
        want_counts = np.bincount(flat, minlength=k["E"])
        assert (counts.cpu().numpy() == want_counts).all()
        incl = np.cumsum(want_counts)
        assert (cursor.cpu().numpy() == incl).all()
        order = order.cpu().numpy()
        assert (np.sort(order) == np.arange(flat.size)).all()
        ids = flat[order]
        assert (np.diff(ids) >= 0).all()
        excl = incl - want_counts
        assert (ids == np.repeat(np.arange(k["E"]), want_counts)).all()  # entity e's range is [excl[e], excl[e + 1])
        assert excl[0] == 0 and incl[-1] == flat.size


# ---- kge_score_spo_bwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SPO_CASES, ids=R.case_id)
def test_spo_bwd_within_bound(case):
    from kge_amd import _lib
    from kge_amd import engine as eng
    k = R.make_case(case)
    want, bound = R.reference(k)
    dev = _device(k)
    n, d, dr = k["n"], k["d"], k["rel"].shape[1]
    ar = _Arena([(n, d, d), (n, dr, dr), (n, d, d)])
    (si, pi, oi), keep = _ix(dev)
    tc = dev["T"].c()
    call = lambda sc: _lib.lib().kge_score_spo_bwd(ctypes.byref(tc), si, pi, oi, n, dev["gout"].data_ptr(), _ptr(sc),
                                                   ar.ptr(0), ar.ptr(1), ar.ptr(2), eng._stream_handle(DEV))
    if dev["scores"] is not None:
        assert call(None) == INVALID_ARG
        torch.cuda.synchronize()
        assert bool((ar.buf.view(torch.int32) == NAN_BITS).all())
    assert call(dev["scores"]) == 0
    torch.cuda.synchronize()
    _check(R.case_id(case), ar, want, bound, ("g_s", "g_p", "g_o"))
    if k["name"] == "transe" and k["l_norm"] == 1.0 and d > 1:  # the planted tie weighs +1, exactly
        g = float(k["gout"][0])
        assert (ar.get(0)[0, 0], ar.get(1)[0, 0], ar.get(2)[0, 0]) == (-g, -g, g)


# ---- kge_score_spo_bwd_accum ---------------------------------------------------------------------------------------------------
def _call_acc(k, dev, ar, scores="own"):
    from kge_amd import _lib
    from kge_amd import engine as eng
    (si, pi, oi), keep = _ix(dev)
    tc = dev["T"].c()
    sc = dev["scores"] if scores == "own" else scores
    return _lib.lib().kge_score_spo_bwd_accum(ctypes.byref(tc), si, pi, oi, k["n"], dev["gout"].data_ptr(), _ptr(sc),
                                              ar.ptr(0), ar.shapes[0][2], ar.ptr(1), ar.shapes[1][2],
                                              eng._stream_handle(DEV))


@pytest.mark.parametrize("case", R.ACC_CASES, ids=R.case_id)
def test_spo_bwd_accum_within_bound(case):
    k = R.make_case(case)
    want, bound = R.reference(k)
    dev = _device(k)
    ar = _grad_arena(k, k["rel"].shape[1])
    if dev["scores"] is not None:
        assert _call_acc(k, dev, ar, None) == INVALID_ARG
    assert _call_acc(k, dev, ar) == 0
    torch.cuda.synchronize()
    _check(R.case_id(case), ar, want, bound)


def test_spo_bwd_accum_unsupported_and_empty_leave_the_gradients_alone():
    for case, rc, n in ((R.ACC_UNSUPPORTED, UNSUPPORTED, None), (R.ACC_CASES[0], 0, 0)):
        k = R.make_case(case)
        dev = _device(k)
        if n is not None:
            k["n"] = n
        dr = k["rel"].shape[1]
        ar = _Arena([(k["E"], k["d"], k["d"]), (k["R"], dr, dr)])
        assert _call_acc(k, dev, ar) == rc
        torch.cuda.synchronize()
        assert bool((ar.buf.view(torch.int32) == NAN_BITS).all())
