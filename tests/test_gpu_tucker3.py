"""The Tucker3 projection kernels (csrc/tucker3.hip) through the C ABI on the GPU: the projection and its backward within
the derived bound of tests/_tucker3_ref.py, and the equalities the canonical arithmetic promises, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import _tucker3_ref as tr

pytestmark = pytest.mark.gpu

DS = (8, 13, 32, 33)            # d = 13: odd widths, the element path; d = 33: N = 1089, a ragged last column tile
DRS = (1, 5, 32, 33, 100)       # one term; short; one K chunk exactly; one past it; the default (not a multiple of 32)
ROWS = (1, 3, 130)              # 130 rows cross the 64- and 128-row tiles
R = 7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


def _pitched(x, ld, dev, misalign=False):
    """x [r, c] as a view with row pitch ld (> c) in a NaN-filled buffer -- and, misaligned, one float off the 16-byte grid"""
    r, c = x.shape
    buf = torch.full((r * ld + 4,), float("nan"), device=dev)
    v = buf[1:1 + r * ld] if misalign else buf[:r * ld]
    v = v.view(r, ld)[:, :c]
    v.copy_(x if torch.is_tensor(x) else torch.from_numpy(x))
    return v


_CASES = {}


def _case(d, dr, rows):
    """parameters, an index with repeats in no order (base row 1 is all zero), the float64 projection: computed once"""
    key = (d, dr, rows)
    if key not in _CASES:
        _, B, W = tr.make_params(2, R, d, dr, 1000 * d + dr)
        rng = np.random.default_rng(d + dr + rows)
        idx = rng.integers(0, R, rows)
        idx[0] = 1
        if rows > 2:
            idx[2] = idx[1]
        _CASES[key] = (B, W, idx, tr.project(B, W, idx))
    return _CASES[key]


def _within(got, ref, what):
    want, e = ref
    got = got.double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want)
    tol = tr.bound(e)
    bad = err > tol
    assert not bad.any(), "{}: {} of {} outside the bound (worst {:.3e} at a bound of {:.3e})".format(
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(tol[bad][err[bad].argmax()]))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("dr", DRS)
def test_projection_within_bound(dev, d, dr):
    from kge_amd import engine
    for rows in ROWS:
        B, W, idx, ref = _case(d, dr, rows)
        Bt, Wt = torch.from_numpy(B).to(dev), torch.from_numpy(W).to(dev)
        out = engine.tucker3_project(Bt, Wt, torch.from_numpy(idx).to(dev))
        _within(out, ref, "projection d={} dr={} rows={}".format(d, dr, rows))
        assert not out[idx == 1].any(), "the zero base row projects to zero"


@pytest.mark.parametrize("d,dr", [(8, 5), (13, 33), (32, 100), (33, 32)])
def test_projection_bit_equalities(dev, d, dr):
    """an element is a pure function of its B row and its W row"""
    from kge_amd import engine
    _, B, W = tr.make_params(2, 130, d, dr, 7 * d + dr)
    Rn = B.shape[0]
    Bt, Wt = torch.from_numpy(B).to(dev), torch.from_numpy(W).to(dev)
    full = engine.tucker3_project(Bt, Wt)  # the range 0 .. R
    ident = torch.arange(Rn, device=dev)
    assert torch.equal(engine.tucker3_project(Bt, Wt, ident), full), "range against the gathered identity"
    assert torch.equal(engine.tucker3_project(Bt, Wt, range(3, 70)), full[3:70]), "a range that starts inside the table"
    rng = np.random.default_rng(d)
    idx = torch.from_numpy(np.concatenate([rng.permutation(Rn)[:67], [5, 5, 129, 0]])).to(dev)
    want = full[idx]
    assert torch.equal(engine.tucker3_project(Bt, Wt, idx), want), "gathered rows, repeats, permuted"
    assert torch.equal(engine.tucker3_project(Bt, Wt, idx.int()), want), "int32 index"
    for dt in (torch.int64, torch.int32):
        buf = torch.full((2 * idx.numel(),), -1, dtype=dt, device=dev)
        buf[::2] = idx.to(dt)
        assert torch.equal(engine.tucker3_project(Bt, Wt, buf[::2]), want), "strided index"
    assert torch.equal(engine.tucker3_project(Bt, Wt, idx[:1]), want[:1]), "one row"
    # ld > width on each operand, and bases one float off the 16-byte grid (the element paths)
    for name, Bv, Wv in (("B pitched", _pitched(B, dr + 4, dev), Wt), ("W pitched", Bt, _pitched(W, dr + 8, dev)),
                         ("B odd pitch, off the grid", _pitched(B, dr + 3, dev, True), Wt),
                         ("W odd pitch, off the grid", Bt, _pitched(W, dr + 1, dev, True))):
        assert torch.equal(engine.tucker3_project(Bv, Wv, idx), want), name
    n = idx.numel()
    for name, o in (("out pitched", _pitched(torch.zeros(n, d * d), d * d + 4, dev)),
                    ("out odd pitch, off the grid", _pitched(torch.zeros(n, d * d), d * d + 3, dev, True))):
        engine.tucker3_project(Bt, Wt, idx, out=o)
        assert torch.equal(o, want), name
        base = o.as_strided((n, o.stride(0)), (o.stride(0), 1), o.storage_offset())
        assert bool(torch.isnan(base[:-1, d * d:]).all()), name + ": nothing written between the rows"


def _backward_case(dev, d, dr, rows):
    from kge_amd import engine
    _, B, W = tr.make_params(2, R, d, dr, 31 * d + dr)
    rng = np.random.default_rng(rows + d)
    idx = rng.integers(0, R, rows)
    idx[0] = 1
    if rows > 2:
        idx[2] = idx[1]  # a repeated index
    g = rng.standard_normal((rows, d * d)).astype(np.float32)
    ref_rows, ref_w = tr.project_bwd(B, W, idx, g)
    Bt, Wt, gt = torch.from_numpy(B).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(g).to(dev)
    it = torch.from_numpy(idx).to(dev)
    what = "d={} dr={} rows={}".format(d, dr, rows)
    g_rows, g_w = engine.tucker3_project_bwd(Bt, Wt, it, gt)
    _within(g_rows, ref_rows, "g_Brows " + what)
    _within(g_w, ref_w, "g_W " + what)
    g_rows2, g_w2 = engine.tucker3_project_bwd(Bt, Wt, it, gt)
    assert torch.equal(g_rows, g_rows2) and torch.equal(g_w, g_w2), "two runs give the same bits " + what
    only_rows, none = engine.tucker3_project_bwd(Bt, Wt, it, gt, want_w=False)
    assert none is None and torch.equal(only_rows, g_rows)
    if rows >= R:  # all rows through the range form
        gr = gt[:R].contiguous()
        ra, wa = engine.tucker3_project_bwd(Bt, Wt, None, gr)
        rb, wb = engine.tucker3_project_bwd(Bt, Wt, torch.arange(R, device=dev), gr)
        assert torch.equal(ra, rb) and torch.equal(wa, wb), "range against the gathered identity " + what


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("dr", DRS)
def test_backward_within_bound(dev, d, dr):
    """g_Brows and g_W at the shapes of the projection test: odd d_r and d^2 take the element loads of the gradient
    products, (rows * d_r) % 4 != 0 their unsplit form"""
    for rows in ROWS:
        _backward_case(dev, d, dr, rows)


def test_backward_split_k(dev):
    """d = 64, d_r = 100, 40 rows: K = 4096 over one output tile, the split-K route of g_Brows"""
    _backward_case(dev, 64, 100, 40)


def test_backward_short_workspace(dev):
    from kge_amd import _lib, engine
    d, dr, n = 64, 100, 40
    _, B, W = tr.make_params(2, R, d, dr, 5)
    Bt, Wt = torch.from_numpy(B).to(dev), torch.from_numpy(W).to(dev)
    tc, _ = engine._tucker3(Bt, Wt, "test")
    L = _lib.lib()
    need = L.kge_tucker3_project_bwd_workspace_bytes(ctypes.byref(tc), n)
    assert need > n * dr * 4, "the split-K partials are part of the workspace at this shape"
    g = torch.zeros(n, d * d, device=dev)
    g_rows, g_w = torch.full((n, dr), 7.0, device=dev), torch.full((d * d, dr), 7.0, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    idx = _lib.KgeIndex(None, _lib.I64, 0, 1)  # rows 0 .. n of a 7-row table: refused before the workspace is looked at
    args = (g.data_ptr(), d * d, g_rows.data_ptr(), dr, g_w.data_ptr(), dr)
    assert L.kge_tucker3_project_bwd(ctypes.byref(tc), idx, n, *args, ws.data_ptr(), need, None) == -1
    ix = torch.zeros(n, dtype=torch.int64, device=dev)
    idx = _lib.KgeIndex(ix.data_ptr(), _lib.I64, 0, 1)
    for wsp, nbytes in ((None, 0), (ws.data_ptr(), need - 1), (None, need)):
        assert L.kge_tucker3_project_bwd(ctypes.byref(tc), idx, n, *args, wsp, nbytes, None) == -5  # KGE_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((g_rows == 7.0).all()) and bool((g_w == 7.0).all()), "a refused call writes nothing"
    assert L.kge_tucker3_project_bwd(ctypes.byref(tc), idx, n, *args, ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert not g_rows.any() and not g_w.any()
