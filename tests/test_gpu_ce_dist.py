"""Fused 1vsAll cross entropy of TransE / RotatE on float32 tables (kge_ce_dist_fwd / kge_ce_dist_bwd, ce_dist.hip)
on the MI355X: the forward against float64 cross entropy of the project's own stored scores and of the oracle's, the
backward against float64 autograd of the reference's op sequence and against the unfused device path, chunkings
against each other, guard rows / columns / workspace tail, the memory bound, and the model level."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle as ko
import torch_port as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (d, E, R, n): ragged everywhere in one column group (the shape of test_backward_matches_torch_autograd); exactly one
# full tile; one row and a second tile with 6 valid columns; several row and column groups; a last tile with ONE valid
# column (half the lanes see only padding); TransE with an odd dimension
SHAPES = [(40, 150, 5, 37), (64, 64, 3, 64), (32, 70, 3, 1), (128, 1037, 13, 203), (64, 64 * 14 + 1, 5, 130)]
CASES = [(name, l_norm, *shape) for shape in SHAPES for name in ("transe", "rotate") for l_norm in (1.0, 2.0)]
CASES += [("transe", 1.0, 33, 150, 5, 37), ("transe", 2.0, 33, 150, 5, 37)]
DIRECTIONS = ("sp", "po")


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ce64(scores, label):
    """float64 (loss_rows, lse) of scores [n, E] with index labels"""
    x = np.asarray(scores, dtype=np.float64)
    mx = x.max(axis=1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    return lse - x[np.arange(len(label)), label], lse


@functools.lru_cache(maxsize=None)
def _case(name, l_norm, d, E, R, n):
    """Inputs and every reference of one case, computed once and shared (never modified): tables, triples, the oracle's
    scores, upstream gradients and the float64 autograd gradients of both directions."""
    # (seed offset 7: a draw in which no float64 q - t of a TransE case is exactly 0 -- with 27 M float32 pairs at the
    # largest shape an exact tie is not rare; _nonzero_differences asserts it)
    rng = np.random.default_rng(7 + 1000 * d + n + int(l_norm))
    ent = rng.standard_normal((E, d)).astype(np.float32)
    dr = d // 2 if name == "rotate" else d
    rel = rng.standard_normal((R, dr)).astype(np.float32)
    s, p, o = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    g_rows = rng.uniform(0.1, 1.0, n).astype(np.float32)
    O = ko.Tables(name, ent, rel, l_norm)
    out = {"ent": ent, "rel": rel, "s": s, "p": p, "o": o, "g_rows": g_rows, "dr": dr}
    for direction in DIRECTIONS:
        a, lab = (s, o) if direction == "sp" else (o, s)
        out["oracle_" + direction] = ko.score_sp(O, a, p) if direction == "sp" else ko.score_po(O, p, a)
        for gname, g in (("rows", g_rows.astype(np.float64)), ("scalar", np.full(n, 0.37))):
            e64 = torch.from_numpy(ent).double().requires_grad_()
            r64 = torch.from_numpy(rel).double().requires_grad_()
            ai, pi = torch.from_numpy(a), torch.from_numpy(p)
            sc = tp.score_sp(name, e64, r64, ai, pi, None, l_norm) if direction == "sp" else \
                tp.score_po(name, e64, r64, pi, ai, None, l_norm)
            rows = torch.nn.functional.cross_entropy(sc, torch.from_numpy(lab), reduction="none")
            (rows * torch.from_numpy(g)).sum().backward()
            out[f"grad64_{direction}_{gname}"] = (e64.grad.numpy(), r64.grad.numpy())
    return out


def _nonzero_differences(c, name, direction):
    """The float64 reference differentiates |q - t| of the float32 table values: no element of q - t, in the float64
    it computes, is exactly 0 (TransE; RotatE's modulus is 0 only where both parts are).  The kernel's float32 q can
    still round onto a t -- its sign(0) = 0 against the reference's +-1 is then part of the error the tolerance bounds."""
    if name != "transe":
        return True
    a, p = (c["s"], c["p"]) if direction == "sp" else (c["o"], c["p"])
    ent, rel = c["ent"].astype(np.float64), c["rel"].astype(np.float64)
    q = ent[a] + rel[p] if direction == "sp" else ent[a] - rel[p]
    return bool(np.all(q[:, None, :] != ent[None, :, :]))


def _tables(eng, name, l_norm, c):
    return eng.Tables(name, _t(c["ent"]), _t(c["rel"]), l_norm)


def _table_grads(c, direction, g_a, g_p, g_t):
    """(entity gradient [E, d], relation gradient [R, dr]) from the kernel's outputs, in float64 on the host"""
    a = c["s"] if direction == "sp" else c["o"]
    ge = g_t.double().cpu().numpy().copy()
    np.add.at(ge, a, g_a.double().cpu().numpy())
    gr = np.zeros((c["rel"].shape[0], c["dr"]))
    np.add.at(gr, c["p"], g_p.double().cpu().numpy())
    return ge, gr


def _close(got, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"{what}: max |err| {err:.3e} scale {scale:.3e}")
    assert err <= 2e-4 * scale, (what, err, scale)


@pytest.mark.parametrize("name,l_norm,d,E,R,n", CASES)
def test_forward_against_stored_scores_and_oracle(eng, name, l_norm, d, E, R, n):
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction in DIRECTIONS:
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        loss, lse = eng.ce_dist_fwd(T, direction, _t(a), _t(c["p"]), _t(lab))
        loss2, lse2 = eng.ce_dist_fwd(T, direction, _t(a), _t(c["p"]), _t(lab))
        assert torch.equal(loss, loss2) and torch.equal(lse, lse2), "two runs differ"
        loss, lse = loss.cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
        assert np.isfinite(loss).all() and np.isfinite(lse).all() and (loss >= 0).all(), direction
        sc = (eng.score_sp(T, _t(a), _t(c["p"])) if direction == "sp" else eng.score_po(T, _t(c["p"]), _t(a))).cpu().numpy()
        assert np.array_equal(sc, c["oracle_" + direction]), "stored scores differ from the oracle's"
        for ref_name, ref in (("stored", sc), ("oracle", c["oracle_" + direction])):
            want_loss, want_lse = _ce64(ref, lab)
            for nm, got, want in (("lse", lse, want_lse), ("loss", loss, want_loss)):
                err = np.abs(got - want)
                tol = 1e-5 + 1e-5 * np.abs(want)
                print(f"{name} L{l_norm:g} {direction} {nm} vs {ref_name}: max err {err.max():.3e} min tol {tol.min():.3e}")
                assert (err <= tol).all(), (direction, ref_name, nm, float(err.max()), int((err > tol).sum()))


def test_forward_strided_int32_repeats_empty_and_bad_label(eng):
    name, l_norm, d, E, R, n = "rotate", 2.0, 40, 150, 5, 37
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    tri = np.stack([c["s"], c["p"], c["o"]], 1)
    tri[5:9] = tri[4]  # repeated rows
    t32 = _t(tri.astype(np.int32))
    loss, lse = eng.ce_dist_fwd(T, "sp", t32[:, 0], t32[:, 1], t32[:, 2])
    loss64, lse64 = eng.ce_dist_fwd(T, "sp", _t(tri[:, 0]), _t(tri[:, 1]), _t(tri[:, 2]))
    assert torch.equal(loss, loss64) and torch.equal(lse, lse64)
    assert torch.equal(loss[5:9], loss[4:5].expand(4))
    # n = 0
    e = torch.zeros(0, dtype=torch.int64, device=DEV)
    l0, s0 = eng.ce_dist_fwd(T, "po", e, e, e)
    assert l0.shape == (0,) and s0.shape == (0,)
    g0 = eng.ce_dist_bwd(T, "po", e, e, e, s0)
    assert g0[0].shape == (0, d) and g0[2].shape == (E, d) and float(g0[2].abs().max()) == 0.0
    # a label out of range: NaN in that row only, lse untouched
    bad = tri[:, 2].copy()
    bad[3], bad[11] = E, -1
    lb, sb = eng.ce_dist_fwd(T, "sp", _t(tri[:, 0]), _t(tri[:, 1]), _t(bad))
    nan = torch.isnan(lb).cpu().numpy()
    assert nan.tolist() == [i in (3, 11) for i in range(n)]
    assert torch.equal(sb, lse64) and torch.equal(lb[~torch.isnan(lb)], loss64[torch.from_numpy(~nan).to(DEV)])


@pytest.mark.parametrize("name,l_norm,d,E,R,n", CASES)
def test_backward_against_float64_autograd_and_the_unfused_path(eng, name, l_norm, d, E, R, n):
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction in DIRECTIONS:
        assert _nonzero_differences(c, name, direction)
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        ai, pi, li = _t(a), _t(c["p"]), _t(lab)
        _, lse = eng.ce_dist_fwd(T, direction, ai, pi, li)
        sc = eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)
        for gname, kw, g in (("rows", {"g_rows": _t(c["g_rows"])}, c["g_rows"].astype(np.float64)),
                             ("scalar", {"g_scalar": 0.37}, np.full(n, np.float64(np.float32(0.37))))):
            g_a, g_p, g_t = eng.ce_dist_bwd(T, direction, ai, pi, li, lse, **kw)
            ge, gr = _table_grads(c, direction, g_a, g_p, g_t)
            want_e, want_r = c[f"grad64_{direction}_{gname}"]
            _close(ge, want_e, f"{name} L{l_norm:g} {direction} {gname} entity vs float64 autograd")
            _close(gr, want_r, f"{name} L{l_norm:g} {direction} {gname} relation vs float64 autograd")
            # the unfused device path fed with gout = g (softmax - onehot) in float64 from the kernel's own scores
            x = sc.double().cpu().numpy()
            _, lse64 = _ce64(x, lab)
            gout = np.exp(x - lse64[:, None])
            gout[np.arange(n), lab] -= 1.0
            gout = (gout * g[:, None]).astype(np.float32)
            u_a, u_p, u_t = eng.score_pairs_bwd(T, direction, ai, pi, None, _t(gout), sc)
            for nm, got, want in (("g_a", g_a, u_a), ("g_p", g_p, u_p), ("g_tgt", g_t, u_t)):
                _close(got.double().cpu().numpy(), want.double().cpu().numpy(),
                       f"{name} L{l_norm:g} {direction} {gname} {nm} vs score_pairs_bwd")


@pytest.mark.parametrize("name,l_norm", [("transe", 1.0), ("transe", 2.0), ("rotate", 1.0), ("rotate", 2.0)])
@pytest.mark.parametrize("d,E,R,n", [(128, 1037, 13, 203), (64, 64 * 14 + 1, 5, 130)])
def test_chunkings_agree(eng, name, l_norm, d, E, R, n):
    """chunk_cols 64, 128 and E rounded up (one chunk): every output within 2e-4 max(1, |want|max) of the single-chunk
    result.  g_tgt is BIT-equal across chunkings: a target row's gradient is one chain over the query rows in order,
    from scores that do not depend on the chunk -- the chunk only decides which launch writes the row."""
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction in DIRECTIONS:
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        ai, pi, li = _t(a), _t(c["p"]), _t(lab)
        _, lse = eng.ce_dist_fwd(T, direction, ai, pi, li)
        one = eng.ce_dist_bwd(T, direction, ai, pi, li, lse, g_rows=_t(c["g_rows"]), chunk_cols=(E + 63) // 64 * 64)
        for cc in (64, 128):
            got = eng.ce_dist_bwd(T, direction, ai, pi, li, lse, g_rows=_t(c["g_rows"]), chunk_cols=cc)
            for nm, x, w in zip(("g_a", "g_p", "g_tgt"), got, one):
                _close(x.double().cpu().numpy(), w.double().cpu().numpy(), f"{name} {direction} chunk {cc} {nm}")
            assert torch.equal(got[2], one[2]), f"g_tgt differs between chunk_cols {cc} and one chunk"


def _raw_call(eng, T, direction, a, p, lab, n, E, d, dr, chunk_cols, g_rows):
    """kge_ce_dist_fwd + kge_ce_dist_bwd through ctypes on outputs and a workspace with guards; returns the guarded
    buffers and the views the calls wrote."""
    from kge_amd import _lib
    from kge_amd._lib import PO_, SP_
    lib = _lib.lib()
    tc = T.c()
    keep = []
    ai, pi, li = (eng._index(x, T.device, keep) for x in (a, p, lab))
    need = lib.kge_ce_dist_workspace_bytes(ctypes.byref(tc), n, chunk_cols)
    assert need > 0 and need % 256 == 0
    S = 7.25  # sentinel
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    rows = torch.full((2, n + 2), S, device=DEV)                    # loss_rows, lse with a guard on either side
    ga = torch.full((n + 2, d + 2), S, device=DEV)
    gp = torch.full((n + 2, dr + 2), S, device=DEV)
    gt = torch.full((E + 2, d), S, device=DEV)                      # g_tgt is dense [E, d]: guard rows
    ga_c, gp_c = torch.empty(n, d, device=DEV), torch.empty(n, dr, device=DEV)
    st = eng._stream(T.device)
    dirc = SP_ if direction == "sp" else PO_
    _lib.check(lib.kge_ce_dist_fwd(ctypes.byref(tc), dirc, ai, pi, li, n, rows[0, 1:].data_ptr(), rows[1, 1:].data_ptr(),
                                   ws.data_ptr(), need, st), "fwd")
    _lib.check(lib.kge_ce_dist_bwd(ctypes.byref(tc), dirc, ai, pi, li, n, rows[1, 1:].data_ptr(), g_rows.data_ptr(), 1.0,
                                   ga_c.data_ptr(), gp_c.data_ptr(), gt[1:].data_ptr(), ws.data_ptr(), need, st), "bwd")
    torch.cuda.synchronize()
    return S, ws, need, rows, gt, ga_c, gp_c


@pytest.mark.parametrize("name,l_norm,d,E,R,n", [("transe", 1.0, 33, 150, 5, 37), ("rotate", 2.0, 64, 64 * 14 + 1, 5, 130),
                                                 ("transe", 2.0, 32, 70, 3, 1)])
def test_guards_and_workspace_tail_are_untouched(eng, name, l_norm, d, E, R, n):
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction, cc in (("sp", 0), ("po", 64)):
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        S, ws, need, rows, gt, ga_c, gp_c = _raw_call(eng, T, direction, _t(a), _t(c["p"]), _t(lab), n, E, d, c["dr"], cc,
                                                      _t(c["g_rows"]))
        assert bool((ws[need:] == 0x5A).all()), "workspace tail written"
        assert bool((rows[:, 0] == S).all()) and bool((rows[:, n + 1] == S).all()), "loss_rows / lse guards"
        assert bool((gt[0] == S).all()) and bool((gt[E + 1] == S).all()), "g_tgt guard rows"
        assert bool(torch.isfinite(gt[1:E + 1]).all()) and not bool((gt[1:E + 1] == S).all(dim=1).any())
        want = eng.ce_dist_bwd(T, direction, _t(a), _t(c["p"]), _t(lab), rows[1, 1:n + 1].contiguous(),
                               g_rows=_t(c["g_rows"]), chunk_cols=cc)
        assert torch.equal(gt[1:E + 1], want[2])
        _close(ga_c.double().cpu().numpy(), want[0].double().cpu().numpy(), "g_a raw vs engine")
        _close(gp_c.double().cpu().numpy(), want[1].double().cpu().numpy(), "g_p raw vs engine")


def test_query_gradients_leave_guard_rows_and_columns(eng):
    """g_a / g_p are dense [n, dim] / [n, rel_dim] outputs: written into the inside of a larger sentinel matrix (row
    pitch = the dense row: the ABI has no pitch for them), the rows before and after stay untouched."""
    from kge_amd import _lib
    name, l_norm, d, E, R, n = "rotate", 1.0, 40, 150, 5, 37
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    ai, pi, li = _t(c["s"]), _t(c["p"]), _t(c["o"])
    _, lse = eng.ce_dist_fwd(T, "sp", ai, pi, li)
    lib, tc, keep = _lib.lib(), T.c(), []
    ix = [eng._index(x, T.device, keep) for x in (ai, pi, li)]
    need = lib.kge_ce_dist_workspace_bytes(ctypes.byref(tc), n, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    S = -3.5
    ga, gp, gt = (torch.full((r + 2, w), S, device=DEV) for r, w in ((n, d), (n, c["dr"]), (E, d)))
    _lib.check(lib.kge_ce_dist_bwd(ctypes.byref(tc), _lib.SP_, *ix, n, lse.data_ptr(), None, 0.5, ga[1:].data_ptr(),
                                   gp[1:].data_ptr(), gt[1:].data_ptr(), ws.data_ptr(), need, eng._stream(T.device)), "bwd")
    torch.cuda.synchronize()
    for nm, x, r in (("g_a", ga, n), ("g_p", gp, n), ("g_tgt", gt, E)):
        assert bool((x[0] == S).all()) and bool((x[r + 1] == S).all()), nm
        assert not bool((x[1:r + 1] == S).any()), nm + ": an element was not written"
    # too small a workspace is refused, nothing written
    assert lib.kge_ce_dist_bwd(ctypes.byref(tc), _lib.SP_, *ix, n, lse.data_ptr(), None, 0.5, ga[1:].data_ptr(),
                               gp[1:].data_ptr(), gt[1:].data_ptr(), ws.data_ptr(), 256, eng._stream(T.device)) == -5


def test_memory_bound_of_a_model_step():
    """n = 256, E = 131,072, d = 16: one [n, E] float32 matrix is 128 MB (the composed path holds several).  The fused
    step raises max_memory_allocated by less than 64 MB over what is held after a warm-up step: the 32 MB score chunk
    (already held: the cached workspace), the 8 MB table gradient, slack."""
    from kge_amd import model as km
    E, R, d, n = 131072, 7, 16, 256
    torch.manual_seed(0)
    m = km.create("transe", E, R, d, device=DEV, fused_dist_loss=True).train()
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    m.loss_sp(s, p, o).sum().backward()  # warm-up: workspace and .grad exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = m.loss_sp(s, p, o).sum()
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"fused step: peak rise {rise / 2**20:.1f} MB over {base / 2**20:.1f} MB held")
    assert torch.isfinite(loss) and rise < 64 * 2**20, rise


@pytest.mark.parametrize("name,l_norm", [("transe", 1.0), ("transe", 2.0), ("rotate", 1.0), ("rotate", 2.0)])
def test_model_level_fused_against_composed(name, l_norm):
    """km.create(..., fused_dist_loss=True) against the same model's composed cross_entropy(score_sp) / score_po:
    loss within 1e-5 max(1, |loss|), parameter gradients within a relative norm error of 1e-4 (the issue's bound, kept:
    the printed errors of both paths against float64 are the record)."""
    from kge_amd import model as km
    E, R, d, n = 3005, 11, 64, 300
    torch.manual_seed(0)
    m = km.create(name, E, R, d, l_norm=l_norm, device=DEV, fused_dist_loss=True).train()
    g = torch.Generator().manual_seed(2)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    we, wr = m.get_s_embedder().weight, m.get_p_embedder().weight
    res = {}
    for fused in (True, False):
        m.fused_dist_loss = fused
        m.zero_grad()
        assert (m._ce_dist_tables() is not None) == fused
        rows = m.loss_sp_po(s, p, o)
        assert rows.shape == (2 * n,)
        total = rows.sum() / n
        total.backward()
        res[fused] = (float(total), we.grad.detach().clone(), wr.grad.detach().clone())
    e64, r64 = we.detach().double().cpu().requires_grad_(), wr.detach().double().cpu().requires_grad_()
    sc, pc, oc = s.cpu(), p.cpu(), o.cpu()
    ce = torch.nn.functional.cross_entropy
    t64 = (ce(tp.score_sp(name, e64, r64, sc, pc, None, l_norm), oc, reduction="sum")
           + ce(tp.score_po(name, e64, r64, pc, oc, None, l_norm), sc, reduction="sum")) / n
    t64.backward()
    (lf, gef, grf), (lc, gec, grc) = res[True], res[False]
    assert abs(lf - lc) <= 1e-5 * max(1.0, abs(lc)), (lf, lc)
    for nm, a, b, w in (("entity", gef, gec, e64.grad), ("relation", grf, grc, r64.grad)):
        rel = float((a - b).norm() / b.norm())
        ef = float((a.double().cpu() - w).norm() / w.norm())
        ec = float((b.double().cpu() - w).norm() / w.norm())
        print(f"{name} L{l_norm:g} {nm}: fused vs composed {rel:.3e}; vs float64: fused {ef:.3e} composed {ec:.3e}")
        assert rel <= 1e-4, (nm, rel, ef, ec)


def test_unsupported_tables_are_refused(eng):
    ent, rel = torch.randn(70, 64, device=DEV), torch.randn(3, 64, device=DEV)
    ix = torch.zeros(4, dtype=torch.int64, device=DEV)
    for T in (eng.Tables("complex", ent, rel), eng.Tables("transe", ent.bfloat16(), rel.bfloat16()),
              eng.Tables("transe", ent, rel, 3.0)):
        assert not eng.ce_dist_supported(T)
        with pytest.raises(RuntimeError):
            eng.ce_dist_fwd(T, "sp", ix, ix, ix)
    assert eng.ce_dist_supported(eng.Tables("transe", ent, rel, 2.0))
    assert not eng.ce_supported(eng.Tables("transe", ent, rel, 2.0))
