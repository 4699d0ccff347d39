"""The frequency-weighted penalty kernels (kge_amd/csrc/wpenalty.hip) on the MI355X through the ctypes binding.

kge_penalty_count: counts equal numpy.bincount exactly (int32 / int64 ids, n = 0, 1, 37, a stride-3 column, an [n, 2]
block with ld = 3, one id repeated n times, an id out of range, with and without the in-wave duplicate merge, with and
without a bitmap).  The four updates: V = 67 rows (rows 0, 31, 32, 63, 64, 66 sit on the bitmap and count word tails),
dim 8 (four floats per lane, n3) and dim 6 (one float per lane; a dense count that is no multiple of 4, quads that span
two rows); parameters, state and the bf16 copy carry the BITS of the float32 restatement (tests/_wpenalty_ref.py);
counts, bitmap and the touched gradient are zero afterwards; rows with a clear bit are bit-identical in every array;
with counts[r] == m on every row the dense entries give the bits of the existing unweighted entries; *value lies within
the derived bound (_wpenalty_ref.value_bound) of the float64 sum.  The largest err / bound seen is
written to profiles/wpenalty_bound.txt."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import _adam_multi_ref as amr
import _sparse_adam_ref as sar
import _touched_ref as tr
import _wpenalty_ref as wr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
V, N = 67, 37
EDGE_ROWS = [0, 31, 32, 63, 64, 66]
KINDS = [("lp", 1, 8), ("lp", 2, 8), ("lp", 3, 8), ("n3_complex", 3, 8), ("lp", 1, 6), ("lp", 2, 6), ("lp", 3, 6)]
WEIGHT, MINUS_CLR, EPS = 0.37, -0.1, 1e-10
LR, BETAS, ADAM_EPS = 0.01, (0.9, 0.999), 1e-8
SENT = 0x7FC12345
_RATIOS = []


@pytest.fixture(scope="module")
def L():
    from kge_amd import _lib
    return _lib


def _ids(rng, n=N):
    ids = rng.integers(0, V, n)
    ids[: min(n, len(EDGE_ROWS))] = EDGE_ROWS[: min(n, len(EDGE_ROWS))]
    if n > 10:
        ids[7:10] = 31  # a repeated row
    return ids.astype(np.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else \
        t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _kind_code(kind):
    return 1 if kind == "lp" else 2


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_counts_equal_bincount_for_every_index_layout(L, dtype, plain):
    from kge_amd import engine
    rng = np.random.default_rng(5)
    cases = []
    for n in (0, 1, N):
        cases.append(("vector", _dev(_ids(rng, n)).to(dtype)))
    tri = np.stack([_ids(rng), rng.integers(0, 5, N), _ids(rng)], axis=1)
    t = _dev(tri).to(dtype)
    cases.append(("stride3", t[:, 2]))
    cases.append(("block_ld3", t[:, 0:2]))
    cases.append(("repeated", torch.full((N,), 64, dtype=dtype, device=DEV)))
    bad = _ids(rng)
    bad[3], bad[4] = V, -1
    cases.append(("out_of_range", _dev(bad).to(dtype)))
    with L.switches(PENALTY_COUNT_PLAIN=1 if plain else 0):
        for name, ids in cases:
            for with_bitmap in (False, True):
                counts = engine.penalty_counts(V, DEV)
                bitmap = engine.touched_bitmap(V, DEV) if with_bitmap else None
                engine.penalty_count(ids, counts, V, bitmap)
                want = wr.counts_of(ids.cpu().numpy(), V)
                got = counts.cpu().numpy().view(np.uint32)
                assert np.array_equal(got, want), (name, with_bitmap)
                if with_bitmap:
                    bm = bitmap.cpu().numpy().view(np.uint32)
                    assert sorted(tr.marked_rows(bm, V)) == sorted(np.nonzero(want)[0].tolist()), name
                    assert not (bm[(V + 31) // 32:]).any()


def _tables(rng, dim, n_state):
    p = rng.standard_normal((V, dim)).astype(np.float32)
    p[1, 0], p[2, 1] = 0.0, -0.0
    g = (0.1 * rng.standard_normal((V, dim))).astype(np.float32)
    st = [np.abs(0.01 * rng.standard_normal((V, dim))).astype(np.float32) for _ in range(n_state)]
    return p, g, st


def _check_value(value, p, counts, kind, pp, workgroups, what):
    got = float(value.cpu()[0])
    want = wr.value_sum64(p, counts, kind, pp)
    bound = wr.value_bound(p, counts, kind, pp, workgroups)
    print(f"{what}: value {got!r} truth {want!r} err {abs(got - want):.3e} bound {bound:.3e}")
    _RATIOS.append((abs(got - want) / bound, what))
    assert abs(got - want) <= bound, (what, got, want, bound)


def _clock_tensor(T):
    rec = struct.pack("<qddff", T, BETAS[0] ** T, BETAS[1] ** T, 0.0, 0.0)
    return torch.frombuffer(bytearray(rec), dtype=torch.int64).to(DEV)


@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind,pp,dim", KINDS)
def test_dense_adagrad_bits_value_and_cleared_counts(L, kind, pp, dim, wd, copy):
    from kge_amd import engine
    rng = np.random.default_rng(11 + dim + pp)
    ids = _ids(rng)
    p, g, (s,) = _tables(rng, dim, 1)
    P, G, S = _dev(p), _dev(g), _dev(s)
    C = torch.full((V, dim), 0x1234, dtype=torch.int16, device=DEV) if copy else None
    counts = engine.penalty_counts(V, DEV)
    engine.penalty_count(_dev(ids), counts, V)
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    seg = L.KgeAdagradSeg(P.data_ptr(), G.data_ptr(), S.data_ptr(), C.data_ptr() if copy else None, V * dim, MINUS_CLR,
                          wd, EPS)
    pen = engine.wpenalty_seg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr(), counts, N)
    L.check(L.lib().kge_adagrad_step_multi_wpenalty(ctypes.byref(seg), ctypes.byref(pen), 1, None), "wpenalty")
    torch.cuda.synchronize()
    c = wr.counts_of(ids, V)
    pn, sn, cn = wr.adagrad_dense(p, g, s, c, N, kind, pp, WEIGHT, MINUS_CLR, wd, EPS)
    assert np.array_equal(_bits(P), pn.view(np.int32)) and np.array_equal(_bits(S), sn.view(np.int32))
    assert np.array_equal(_bits(G), g.view(np.int32))  # (the dense route reads the gradient only)
    if copy:
        assert np.array_equal(_bits(C), cn)
    assert not counts.any()
    _check_value(value, p, c, kind, pp, 1, f"adagrad dense {kind} p={pp} dim={dim}")


@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind,pp,dim", KINDS)
def test_dense_adam_bits_value_and_cleared_counts(L, kind, pp, dim, wd, copy):
    from kge_amd import engine
    rng = np.random.default_rng(23 + dim + pp)
    ids = _ids(rng)
    p, g, (a, b) = _tables(rng, dim, 2)
    P, G, A, B = _dev(p), _dev(g), _dev(a), _dev(b)
    C = torch.full((V, dim), 0x1234, dtype=torch.int16, device=DEV) if copy else None
    clock = _clock_tensor(3)
    counts = engine.penalty_counts(V, DEV)
    engine.penalty_count(_dev(ids), counts, V)
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    seg = L.KgeAdamSeg(P.data_ptr(), G.data_ptr(), A.data_ptr(), B.data_ptr(), C.data_ptr() if copy else None,
                       clock.data_ptr(), V * dim, LR, BETAS[0], BETAS[1], wd, ADAM_EPS)
    pen = engine.wpenalty_seg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr(), counts, N)
    L.check(L.lib().kge_adam_step_multi_wpenalty(ctypes.byref(seg), ctypes.byref(pen), 1, None), "wpenalty")
    torch.cuda.synchronize()
    c = wr.counts_of(ids, V)
    pn, an, bn, cn, ck = wr.adam_dense(p, g, a, b, amr.clock_seed(3, *BETAS), LR, BETAS[0], BETAS[1], c, N, kind, pp,
                                       WEIGHT, wd, ADAM_EPS)
    assert np.array_equal(_bits(P), pn.view(np.int32))
    assert np.array_equal(_bits(A), an.view(np.int32)) and np.array_equal(_bits(B), bn.view(np.int32))
    assert clock.cpu().numpy().tobytes() == amr.clock_bytes(ck)
    if copy:
        assert np.array_equal(_bits(C), cn)
    assert not counts.any()
    _check_value(value, p, c, kind, pp, 1, f"adam dense {kind} p={pp} dim={dim}")


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("kind,pp,dim", KINDS)
def test_full_counts_give_the_bits_of_the_unweighted_entry(L, opt, kind, pp, dim):
    """counts[r] == m on every row: f_r == weight exactly, so the weighted entries ARE the unweighted ones."""
    from kge_amd import engine
    rng = np.random.default_rng(31 + dim + pp)
    p, g, (a, b) = _tables(rng, dim, 2)
    out = []
    for weighted in (False, True):
        P, G, A, B = _dev(p), _dev(g), _dev(a), _dev(b)
        value = torch.zeros(1, dtype=torch.float64, device=DEV)
        counts = torch.full((V,), N, dtype=torch.int32, device=DEV)
        clock = _clock_tensor(0)
        if opt == "adagrad":
            seg = L.KgeAdagradSeg(P.data_ptr(), G.data_ptr(), A.data_ptr(), None, V * dim, MINUS_CLR, 0.01, EPS)
        else:
            seg = L.KgeAdamSeg(P.data_ptr(), G.data_ptr(), A.data_ptr(), B.data_ptr(), None, clock.data_ptr(), V * dim,
                               LR, BETAS[0], BETAS[1], 0.01, ADAM_EPS)
        if weighted:
            pen = engine.wpenalty_seg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr(), counts, N)
            fn = L.lib().kge_adagrad_step_multi_wpenalty if opt == "adagrad" else L.lib().kge_adam_step_multi_wpenalty
        else:
            pen = L.KgePenaltySeg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr())
            fn = L.lib().kge_adagrad_step_multi_penalty if opt == "adagrad" else L.lib().kge_adam_step_multi
        L.check(fn(ctypes.byref(seg), ctypes.byref(pen), 1, None), "step")
        torch.cuda.synchronize()
        out.append((_bits(P), _bits(A), _bits(B)))
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def _touched_inputs(rng, dim, n_state):
    """Marked rows carry real values and a gradient; every other row sentinels (parameter, state) and a zero gradient."""
    ids = _ids(rng)
    marked = sorted(set(ids.tolist()) | {5})  # row 5: marked by the backward, not among the penalty's indexes
    p = np.full((V, dim), SENT, np.uint32).view(np.float32).copy()
    st = [np.full((V, dim), SENT, np.uint32).view(np.float32).copy() for _ in range(n_state)]
    g = np.zeros((V, dim), np.float32)
    rp, rg, rst = _tables(rng, dim, n_state)
    p[marked], g[marked] = rp[marked], rg[marked]
    for s, r in zip(st, rst):
        s[marked] = r[marked]
    return ids, marked, p, g, st


@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("opt", ["adagrad", "sparse_adam"])
@pytest.mark.parametrize("kind,pp,dim", KINDS)
def test_touched_rows_bits_clearing_and_untouched_rows(L, kind, pp, dim, opt, copy):
    from kge_amd import engine
    rng = np.random.default_rng(47 + dim + pp)
    ids, marked, p, g, st = _touched_inputs(rng, dim, 1 if opt == "adagrad" else 2)
    P, G = _dev(p), _dev(g)
    ST = [_dev(s) for s in st]
    c0 = np.full((V, dim), 0xBEEF, np.uint16)
    if copy:
        c0[marked] = wr.orf.bf16_rne_bits(p[marked].reshape(-1)).reshape(len(marked), dim)
    C = _dev(c0.view(np.int16)) if copy else None
    counts = engine.penalty_counts(V, DEV)
    bitmap = engine.touched_bitmap(V, DEV)
    engine.penalty_count(_dev(ids), counts, V, bitmap)
    engine.touched_mark(torch.tensor([5], device=DEV), bitmap, V)
    bm0 = bitmap.cpu().numpy().view(np.uint32).copy()
    assert sorted(tr.marked_rows(bm0, V)) == marked
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    pen = engine.wpenalty_seg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr(), counts, N)
    c = wr.counts_of(ids, V)
    if opt == "adagrad":
        engine.adagrad_step_touched_wpenalty(P, G, ST[0], bitmap, MINUS_CLR, EPS, pen, C)
        pn, gn, sn, cn = wr.adagrad_touched(p, g, st[0], bm0, c, N, kind, pp, WEIGHT, MINUS_CLR, EPS,
                                            c0 if copy else None)
        states = [sn]
    else:
        clock = _clock_tensor(7)
        engine.sparse_adam_step_touched_wpenalty(P, G, ST[0], ST[1], bitmap, clock, LR, BETAS[0], BETAS[1], ADAM_EPS,
                                                 pen, C)
        pn, gn, an, bn, cn, ck = wr.sparse_adam_touched(p, g, st[0], st[1], bm0, sar.clock_seed(7, *BETAS), LR, BETAS[0],
                                                        BETAS[1], c, N, kind, pp, WEIGHT, ADAM_EPS, c0 if copy else None)
        states = [an, bn]
        assert clock.cpu().numpy().tobytes() == sar.clock_bytes(ck)
    torch.cuda.synchronize()
    # whole arrays: the marked rows carry the restatement's bits, every other row its sentinel
    assert np.array_equal(_bits(P), pn.view(np.int32))
    for T, s in zip(ST, states):
        assert np.array_equal(_bits(T), s.view(np.int32))
    if copy:
        assert np.array_equal(_bits(C), cn)
    assert not G.any() and not bitmap.any() and not counts.any()
    unmarked = [r for r in range(V) if r not in marked]
    assert np.array_equal(_bits(P)[unmarked], p.view(np.int32)[unmarked])
    _check_value(value, p[marked], c[marked], kind, pp, 1, f"{opt} touched {kind} p={pp} dim={dim}")


def test_several_workgroups_own_disjoint_rows(L):
    """300 rows of width 8: three workgroups of the dense kernel (128 rows each), two of the touched-row kernel (256)."""
    from kge_amd import engine
    V2, dim, n = 300, 8, 500
    rng = np.random.default_rng(77)
    ids = rng.integers(0, V2, n).astype(np.int64)
    ids[:6] = [0, 127, 128, 255, 256, 299]
    c = wr.counts_of(ids, V2)
    p = rng.standard_normal((V2, dim)).astype(np.float32)
    g = (0.1 * rng.standard_normal((V2, dim))).astype(np.float32)
    s = np.abs(0.01 * rng.standard_normal((V2, dim))).astype(np.float32)
    # dense
    P, G, S = _dev(p), _dev(g), _dev(s)
    counts = engine.penalty_counts(V2, DEV)
    engine.penalty_count(_dev(ids), counts, V2)
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    seg = L.KgeAdagradSeg(P.data_ptr(), G.data_ptr(), S.data_ptr(), None, V2 * dim, MINUS_CLR, 0.0, EPS)
    pen = engine.wpenalty_seg(2, 3, WEIGHT, dim, value.data_ptr(), counts, n)
    L.check(L.lib().kge_adagrad_step_multi_wpenalty(ctypes.byref(seg), ctypes.byref(pen), 1, None), "wpenalty")
    pn, sn, _ = wr.adagrad_dense(p, g, s, c, n, "n3_complex", 3, WEIGHT, MINUS_CLR, 0.0, EPS)
    assert np.array_equal(_bits(P), pn.view(np.int32)) and np.array_equal(_bits(S), sn.view(np.int32))
    assert not counts.any()
    got, want = float(value.cpu()[0]), wr.value_sum64(p, c, "n3_complex", 3)
    assert abs(got - want) <= wr.value_bound(p, c, "n3_complex", 3, 3)
    # touched rows: the gradient lives on the counted rows
    g2 = np.where((c != 0).reshape(-1, 1), g, np.float32(0)).astype(np.float32)
    P, G, S = _dev(p), _dev(g2), _dev(s)
    bitmap = engine.touched_bitmap(V2, DEV)
    engine.penalty_count(_dev(ids), counts, V2, bitmap)
    bm0 = bitmap.cpu().numpy().view(np.uint32).copy()
    value.zero_()
    pen = engine.wpenalty_seg(1, 2, WEIGHT, dim, value.data_ptr(), counts, n)
    engine.adagrad_step_touched_wpenalty(P, G, S, bitmap, MINUS_CLR, EPS, pen)
    pn, gn, sn, _ = wr.adagrad_touched(p, g2, s, bm0, c, n, "lp", 2, WEIGHT, MINUS_CLR, EPS)
    assert np.array_equal(_bits(P), pn.view(np.int32)) and np.array_equal(_bits(S), sn.view(np.int32))
    assert not G.any() and not bitmap.any() and not counts.any()
    got, want = float(value.cpu()[0]), wr.value_sum64(p, c, "lp", 2)
    assert abs(got - want) <= wr.value_bound(p, c, "lp", 2, 2)


def _rows_inputs(rng, rows, dim, n):
    ids = rng.integers(0, rows, n).astype(np.int64)
    ids[:2] = [0, rows - 1]
    p = rng.standard_normal((rows, dim)).astype(np.float32)
    g = (0.1 * rng.standard_normal((rows, dim))).astype(np.float32)
    s = np.abs(0.01 * rng.standard_normal((rows, dim))).astype(np.float32)
    return ids, wr.counts_of(ids, rows), p, g, s


@pytest.mark.parametrize("dim,kind,pp", [(72, "n3_complex", 3), (264, "n3_complex", 3), (264, "lp", 3)])
def test_wide_rows_lane_groups_of_32_and_64_and_four_rows_per_workgroup(L, dim, kind, pp):
    """dim 72: 18 quads per row, groups of 32 lanes; dim 264: 66 quads, groups of 64 lanes and two trips per row; the
    dense kernel owns 4 rows per workgroup at dim 264 (17 workgroups) and 12 at dim 72."""
    from kge_amd import engine
    rng = np.random.default_rng(dim + pp)
    ids, c, p, g, s = _rows_inputs(rng, V, dim, N)
    P, G, S = _dev(p), _dev(g), _dev(s)
    counts = engine.penalty_counts(V, DEV)
    engine.penalty_count(_dev(ids), counts, V)
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    seg = L.KgeAdagradSeg(P.data_ptr(), G.data_ptr(), S.data_ptr(), None, V * dim, MINUS_CLR, 0.0, EPS)
    pen = engine.wpenalty_seg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr(), counts, N)
    L.check(L.lib().kge_adagrad_step_multi_wpenalty(ctypes.byref(seg), ctypes.byref(pen), 1, None), "wpenalty")
    pn, sn, _ = wr.adagrad_dense(p, g, s, c, N, kind, pp, WEIGHT, MINUS_CLR, 0.0, EPS)
    assert np.array_equal(_bits(P), pn.view(np.int32)) and np.array_equal(_bits(S), sn.view(np.int32))
    assert not counts.any()
    _check_value(value, p, c, kind, pp, 17, f"adagrad dense {kind} p={pp} dim={dim}")
    g2 = np.where((c != 0).reshape(-1, 1), g, np.float32(0)).astype(np.float32)
    for opt in ("adagrad", "sparse_adam"):
        P, G, S, S2 = _dev(p), _dev(g2), _dev(s), _dev(s)
        bitmap = engine.touched_bitmap(V, DEV)
        engine.penalty_count(_dev(ids), counts, V, bitmap)
        bm0 = bitmap.cpu().numpy().view(np.uint32).copy()
        value.zero_()
        pen = engine.wpenalty_seg(_kind_code(kind), pp, WEIGHT, dim, value.data_ptr(), counts, N)
        if opt == "adagrad":
            engine.adagrad_step_touched_wpenalty(P, G, S, bitmap, MINUS_CLR, EPS, pen)
            pn, _gn, sn, _ = wr.adagrad_touched(p, g2, s, bm0, c, N, kind, pp, WEIGHT, MINUS_CLR, EPS)
            assert np.array_equal(_bits(S), sn.view(np.int32))
        else:
            clock = _clock_tensor(0)
            engine.sparse_adam_step_touched_wpenalty(P, G, S, S2, bitmap, clock, LR, BETAS[0], BETAS[1], ADAM_EPS, pen)
            pn, _gn, an, bn, _c, _ck = wr.sparse_adam_touched(p, g2, s, s, bm0, sar.clock_seed(0, *BETAS), LR, BETAS[0],
                                                              BETAS[1], c, N, kind, pp, WEIGHT, ADAM_EPS)
            assert np.array_equal(_bits(S), an.view(np.int32)) and np.array_equal(_bits(S2), bn.view(np.int32))
        assert np.array_equal(_bits(P), pn.view(np.int32))
        assert not G.any() and not bitmap.any() and not counts.any()
        _check_value(value, p, c, kind, pp, 1, f"{opt} touched {kind} p={pp} dim={dim}")


@pytest.mark.parametrize("opt", ["adagrad", "sparse_adam"])
def test_n3_on_the_one_float_path_of_the_touched_kernels(L, opt):
    """dim 8 in arrays of pitch 9: no row but the first starts on 16 bytes, so the lanes take one float each and pair
    column c with column c + 4."""
    from kge_amd import engine
    rng = np.random.default_rng(61)
    ids, c, p, g, s = _rows_inputs(rng, V, 8, N)
    g2 = np.where((c != 0).reshape(-1, 1), g, np.float32(0)).astype(np.float32)

    def pitched(a):
        whole = torch.full((V, 9), float("nan"), device=DEV)
        whole[:, :8] = _dev(a)
        return whole, whole[:, :8]
    (wP, P), (wG, G), (wS, S), (wS2, S2) = pitched(p), pitched(g2), pitched(s), pitched(s)
    wG[:, 8] = 0
    counts, bitmap = engine.penalty_counts(V, DEV), engine.touched_bitmap(V, DEV)
    engine.penalty_count(_dev(ids), counts, V, bitmap)
    bm0 = bitmap.cpu().numpy().view(np.uint32).copy()
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    pen = engine.wpenalty_seg(2, 3, WEIGHT, 8, value.data_ptr(), counts, N)
    if opt == "adagrad":
        engine.adagrad_step_touched_wpenalty(P, G, S, bitmap, MINUS_CLR, EPS, pen)
        pn, _gn, sn, _ = wr.adagrad_touched(p, g2, s, bm0, c, N, "n3_complex", 3, WEIGHT, MINUS_CLR, EPS)
    else:
        clock = _clock_tensor(0)
        engine.sparse_adam_step_touched_wpenalty(P, G, S, S2, bitmap, clock, LR, BETAS[0], BETAS[1], ADAM_EPS, pen)
        pn, _gn, sn, bn, _c, _ck = wr.sparse_adam_touched(p, g2, s, s, bm0, sar.clock_seed(0, *BETAS), LR, BETAS[0],
                                                          BETAS[1], c, N, "n3_complex", 3, WEIGHT, ADAM_EPS)
        assert np.array_equal(_bits(S2), bn.view(np.int32))
    assert np.array_equal(_bits(P), pn.view(np.int32)) and np.array_equal(_bits(S), sn.view(np.int32))
    assert torch.isnan(wP[:, 8]).all() and torch.isnan(wS[:, 8]).all()   # the pitch padding is not written
    assert not G.any() and not bitmap.any() and not counts.any()
    _check_value(value, p, c, "n3_complex", 3, 1, f"{opt} touched n3 scalar path")


def test_a_plain_segment_next_to_a_weighted_one_of_odd_width_over_two_workgroups(L):
    """One dense launch, two segments: kind 0 (1030 elements: the plain update and its scalar tail) and a weighted lp
    term on 300 rows of width 6 -- 168 rows per workgroup, two workgroups, quads that span two rows."""
    from kge_amd import engine
    rng = np.random.default_rng(83)
    p0, g0, s0 = (rng.standard_normal(1030).astype(np.float32) for _ in range(3))
    s0 = np.abs(s0)
    ids, c, p1, g1, s1 = _rows_inputs(rng, 300, 6, 500)
    T = [_dev(x) for x in (p0, g0, s0, p1, g1, s1)]
    counts = engine.penalty_counts(300, DEV)
    engine.penalty_count(_dev(ids), counts, 300)
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    segs = (L.KgeAdagradSeg * 2)(
        L.KgeAdagradSeg(T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), None, 1030, MINUS_CLR, 0.01, EPS),
        L.KgeAdagradSeg(T[3].data_ptr(), T[4].data_ptr(), T[5].data_ptr(), None, 1800, MINUS_CLR, 0.0, EPS))
    pens = (L.KgeWPenaltySeg * 2)(engine.wpenalty_seg(0, 0, 0.0, 0, None, None, 0),
                                  engine.wpenalty_seg(1, 3, WEIGHT, 6, value.data_ptr(), counts, 500))
    L.check(L.lib().kge_adagrad_step_multi_wpenalty(segs, pens, 2, None), "wpenalty")
    pn0, sn0 = wr.orf.adagrad(p0, g0, s0, MINUS_CLR, 0.01, EPS)
    pn1, sn1, _ = wr.adagrad_dense(p1, g1, s1, c, 500, "lp", 3, WEIGHT, MINUS_CLR, 0.0, EPS)
    assert np.array_equal(_bits(T[0]), pn0.view(np.int32)) and np.array_equal(_bits(T[2]), sn0.view(np.int32))
    assert np.array_equal(_bits(T[3]), pn1.view(np.int32)) and np.array_equal(_bits(T[5]), sn1.view(np.int32))
    assert not counts.any()
    _check_value(value, p1, c, "lp", 3, 2, "adagrad dense lp p=3 dim=6, two workgroups")


def test_optimizer_classes_fold_count_and_clear(L):
    """kge_amd.optim: set_penalty(weighted=True) + count_penalty + step on Adagrad (dense and touched rows), the
    device-step Adam and SparseAdam; penalty_value is weight / p / m * value; skip_penalties_once leaves zero counts."""
    from kge_amd import optim
    rng = np.random.default_rng(3)
    ids = _dev(_ids(rng))
    c = wr.counts_of(ids.cpu().numpy(), V)
    for name in ("adagrad", "adam", "adagrad_touched", "sparse_adam"):
        w0 = rng.standard_normal((V, 8)).astype(np.float32)
        g0 = (0.1 * rng.standard_normal((V, 8))).astype(np.float32)
        w = torch.nn.Parameter(_dev(w0))
        if name == "adagrad" or name == "adagrad_touched":
            opt = optim.Adagrad([w], lr=0.1)
        elif name == "adam":
            opt = optim.Adam([w], lr=0.01, device_step=True)
        else:
            opt = optim.SparseAdam([w], lr=0.01)
        touched = name in ("adagrad_touched", "sparse_adam")
        if touched:
            pair = opt.enable_touched_rows(w)
        opt.set_penalty(w, "lp", 3, WEIGHT, weighted=True)
        for skip in (False, True):
            before = w.detach().cpu().numpy().copy()
            if touched:
                mask = _dev(c != 0)
                pair[0][mask] = _dev(g0)[mask]
                if name == "sparse_adam":
                    pair.pending = True
            else:
                w.grad = _dev(g0)
            opt.count_penalty(w, ids, N)
            assert np.array_equal(opt.penalty_counts(w).cpu().numpy().view(np.uint32), c)
            if skip:
                opt.skip_penalties_once()
            opt.step()
            torch.cuda.synchronize()
            assert not opt.penalty_counts(w).any(), (name, skip)
            if not skip:
                want = WEIGHT / 3 / N * wr.value_sum64(before, c, "lp", 3)
                assert abs(float(opt.penalty_value(w)) - want) <= 1e-5 * want, name
    # SparseAdam: a count with no backward behind it still sets the pair pending, and step() clears counts and bits
    opt.count_penalty(w, ids, N)
    assert pair.pending
    opt.step()
    assert not opt.penalty_counts(w).any() and not pair[1].any()
    with pytest.raises(ValueError):
        optim.Adam([torch.nn.Parameter(_dev(w0))]).set_penalty(w, "lp", 2, 0.1, weighted=True)
    with pytest.raises(ValueError):
        optim.Adagrad([w]).set_penalty(w, "lp", 2, 0.1, times=2.0, weighted=True)


def test_write_the_largest_ratio_to_profiles():
    """(runs last in this module) profiles/wpenalty_bound.txt: the largest observed err / bound of the value checks."""
    assert _RATIOS, "the value checks ran before this test"
    worst = max(_RATIOS)
    assert worst[0] <= 1.0
    with open(os.path.join(ROOT, "profiles", "wpenalty_bound.txt"), "w") as f:
        f.write("kge_*_wpenalty: |device value - float64 sum| / derived bound (tests/test_gpu_wpenalty.py)\n")
        f.write(f"checks {len(_RATIOS)}  largest ratio {worst[0]:.4f}  ({worst[1]})\n")
