"""Fused 1vsAll cross entropy of ComplEx / DistMult on FLOAT32 tables (kge_ce_f32_fwd / kge_ce_f32_bwd, ce_f32.hip) on
the MI355X: the forward against float64 cross entropy of the project's own stored scores and of the oracle's, the
backward against float64 autograd and against the composed device path (score_sp -> float32 cross_entropy -> autograd
through kge_score_pairs_bwd), chunkings against each other, guards, unsupported tables, the memory bound, the model.

The backward's bound is not fixed in advance: per case the COMPOSED path's own max-abs error against float64 is
measured, and the fused path is allowed 4 x that (another summation order on the same products and operand precision).
Measured on an MI355X over the 96 comparisons below (max |err| / max(1, |want|max), entity and relation table
gradients): composed 1.96e-8 .. 1.06e-6, fused at most 1.04e-6, fused / composed at most 2.60; the bound 4 x composed was
therefore between 7.8e-8 and 4.3e-6.  The composed path's own error -- kge_score_pairs_bwd on
float32 tables, the yardstick here -- is asserted against a derived rounding bound in tests/test_gpu_pairs_bwd.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle as ko
import torch_port as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (d, E, R, n, ent_ld): a ragged single row tile and a second column tile with 22 valid columns; exactly one full tile;
# one row and a tile with ONE valid column; a K tail inside a chunk (hh = 20), two row tiles and 18 column groups of ONE
# tile each, the last with one valid column; four K chunks, several row and column tiles.  One case has ent_ld > d.
# (The forward walks more than one column tile per workgroup only where a table has more than min(256, 1024 / row
# groups) column tiles: WALK below.)
SHAPES = [(16, 150, 5, 37, 16), (64, 128, 3, 128, 64), (8, 129, 3, 1, 8), (40, 128 * 17 + 1, 5, 130, 48),
          (128, 1037, 13, 203, 128)]
# 301 column tiles, two row tiles: the forward's workgroups walk TWO column tiles each (151 groups per row), the last
# group is short -- one tile, which holds ONE valid column.  Labels sit in the second tile of the first, of the second
# and of the last full group, and in the short group (_case).  The running (max, sum) carried from tile to tile, the
# reuse of the operand buffers, the end of a short group and the merge's group index are all compared with float64 here.
WALK = (8, 128 * 300 + 1, 3, 130, 8)
CASES = [(name, *shape) for shape in SHAPES + [WALK] for name in ("complex", "distmult")]
DIRECTIONS = ("sp", "po")
EPS = 2.0 ** -24  # half a float32 ulp at the scale the errors are taken relative to: the floor of a measured error


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ce64(scores, label):
    x = np.asarray(scores, dtype=np.float64)
    mx = x.max(axis=1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    return lse - x[np.arange(len(label)), label], lse


@functools.lru_cache(maxsize=None)
def _case(name, d, E, R, n, ld):
    """Inputs and every reference of one case, computed once and shared (never modified)."""
    rng = np.random.default_rng(11 + 1000 * d + n)
    ent = (0.5 * rng.standard_normal((E, d))).astype(np.float32)
    rel = (0.5 * rng.standard_normal((R, d))).astype(np.float32)
    s, p, o = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    # labels at the table's ends, on either side of a tile edge, in the fourth tile and in the last tile but one
    for k, col in enumerate((0, E - 1, 127, 128, 128 * 3 + 5, (E - 1) // 128 * 128 - 121)):
        if k < n and 0 <= col < E:
            o[k] = s[(k + 2) % n] = min(col, E - 1)
    if n > 8:
        s[7] = s[6]  # a repeated query entity
        o[8] = o[6]
    g_rows = rng.uniform(0.1, 1.0, n).astype(np.float32)
    O = ko.Tables(name, ent, rel)
    out = {"ent": ent, "rel": rel, "s": s, "p": p, "o": o, "g_rows": g_rows}
    for direction in DIRECTIONS:
        a, lab = (s, o) if direction == "sp" else (o, s)
        out["oracle_" + direction] = ko.score_sp(O, a, p) if direction == "sp" else ko.score_po(O, p, a)
        for gname, g in (("rows", g_rows.astype(np.float64)), ("scalar", np.full(n, np.float64(np.float32(0.37))))):
            e64 = torch.from_numpy(ent).double().requires_grad_()
            r64 = torch.from_numpy(rel).double().requires_grad_()
            ai, pi = torch.from_numpy(a), torch.from_numpy(p)
            sc = tp.score_sp(name, e64, r64, ai, pi) if direction == "sp" else tp.score_po(name, e64, r64, pi, ai)
            rows = torch.nn.functional.cross_entropy(sc, torch.from_numpy(lab), reduction="none")
            (rows * torch.from_numpy(g)).sum().backward()
            out[f"grad64_{direction}_{gname}"] = (e64.grad.numpy(), r64.grad.numpy())
    return out


def _tables(eng, name, c, ld):
    ent = _t(c["ent"])
    if ld > ent.shape[1]:  # rows on a wider pitch: a view into a [E, ld] buffer of NaN
        buf = torch.full((ent.shape[0], ld), float("nan"), device=DEV)
        buf[:, :ent.shape[1]] = ent
        ent = buf[:, :c["ent"].shape[1]]
    return eng.Tables(name, ent, _t(c["rel"]))


def _table_grads(c, direction, g_a, g_p, g_t):
    a = c["s"] if direction == "sp" else c["o"]
    ge = g_t.double().cpu().numpy().copy()
    np.add.at(ge, a, g_a.double().cpu().numpy())
    gr = np.zeros(c["rel"].shape)
    np.add.at(gr, c["p"], g_p.double().cpu().numpy())
    return ge, gr


def _err(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _composed(eng, T, c, direction, g, n):
    """The composed device path: score_sp / score_po -> float32 cross_entropy -> autograd -> kge_score_pairs_bwd"""
    a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
    ai, pi = _t(a), _t(c["p"])
    sc = (eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)).clone().requires_grad_()
    rows = torch.nn.functional.cross_entropy(sc, _t(lab), reduction="none")
    (rows * g).sum().backward()
    return eng.score_pairs_bwd(T, direction, ai, pi, None, sc.grad.contiguous(), sc.detach())


@pytest.mark.parametrize("name,d,E,R,n,ld", CASES)
def test_forward_against_stored_scores_and_oracle(eng, name, d, E, R, n, ld):
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    assert eng.ce_f32_supported(T)
    if (d, E, R, n, ld) == WALK:  # the library's own sizes say so: 151 record groups per row = two tiles per workgroup
        from kge_amd import _lib
        al = lambda b: -(-b // 256) * 256
        fixed = _lib.lib().kge_ce_f32_workspace_bytes(ctypes.byref(T.c()), n, 128) - 4 * n * 128
        assert fixed == al(12 * n * 151) + 2 * al(4 * n * d) + al(32 * 4 * n * d), fixed
        assert 128 in c["o"] and 128 * 3 + 5 in c["o"] and 128 * 299 + 7 in c["o"] and E - 1 in c["o"]
    for direction in DIRECTIONS:
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        loss, lse = eng.ce_f32_fwd(T, direction, _t(a), _t(c["p"]), _t(lab))
        loss2, lse2 = eng.ce_f32_fwd(T, direction, _t(a), _t(c["p"]), _t(lab))
        assert torch.equal(loss, loss2) and torch.equal(lse, lse2), "two runs differ"
        loss, lse = loss.cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
        assert np.isfinite(loss).all() and np.isfinite(lse).all() and (loss >= 0).all(), direction
        sc = (eng.score_sp(T, _t(a), _t(c["p"])) if direction == "sp" else eng.score_po(T, _t(c["p"]), _t(a))).cpu().numpy()
        assert np.array_equal(sc, c["oracle_" + direction]), "stored scores differ from the oracle's"
        for ref_name, want_sc in (("stored", sc), ("oracle", c["oracle_" + direction])):
            want_loss, want_lse = _ce64(want_sc, lab)
            for nm, got, want in (("lse", lse, want_lse), ("loss", loss, want_loss)):
                err = np.abs(got - want)
                tol = 1e-5 + 1e-5 * np.abs(want)   # (the bound of tests/test_gpu_ce_dist.py for the same comparison)
                print(f"{name} d{d} E{E} {direction} {nm} vs {ref_name}: max err {err.max():.3e} min tol {tol.min():.3e}")
                assert (err <= tol).all(), (direction, ref_name, nm, float(err.max()), int((err > tol).sum()))


@pytest.mark.parametrize("name,d,E,R,n,ld", CASES)
def test_backward_against_float64_autograd_and_the_composed_path(eng, name, d, E, R, n, ld):
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    for direction in DIRECTIONS:
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        ai, pi, li = _t(a), _t(c["p"]), _t(lab)
        _, lse = eng.ce_f32_fwd(T, direction, ai, pi, li)
        for gname, kw, g in (("rows", {"g_rows": _t(c["g_rows"])}, _t(c["g_rows"])),
                             ("scalar", {"g_scalar": 0.37}, torch.full((n,), 0.37, device=DEV))):
            want_e, want_r = c[f"grad64_{direction}_{gname}"]
            fe, fr = _table_grads(c, direction, *eng.ce_f32_bwd(T, direction, ai, pi, li, lse, **kw))
            ce, cr = _table_grads(c, direction, *_composed(eng, T, c, direction, g, n))
            for nm, f, cm, w in (("entity", fe, ce, want_e), ("relation", fr, cr, want_r)):
                ef, ec, efc = _err(f, w), _err(cm, w), _err(f, cm)
                print(f"BWD {name} d{d} E{E} n{n} {direction} {gname} {nm}: vs float64 fused {ef:.3e} composed {ec:.3e} "
                      f"bound {4 * ec:.3e}; fused vs composed {efc:.3e}")
                bound = 4 * max(ec, EPS)
                assert ef <= bound, (nm, ef, ec)
                assert efc <= bound + ec, (nm, efc, ec)   # (triangle: both within their bound of float64)


@pytest.mark.parametrize("name", ["complex", "distmult"])
@pytest.mark.parametrize("d,E,R,n,ld", [(128, 1037, 13, 203, 128), (40, 128 * 17 + 1, 5, 130, 48)])
def test_chunkings_agree(eng, name, d, E, R, n, ld):
    """chunk_cols 128, 256 and 0 (here: one chunk): g_tgt BIT-equal across the three (a target row's gradient is one
    product over all n queries, whatever launch writes it); g_a / g_p bit-equal across two runs of one chunking.
    Across chunkings the comparison made is: the table gradients of EACH chunking within the backward's bound of float64
    (4 x the composed path's error), and of each chunked run within twice that bound of the one-chunk run (what the
    first gives by the triangle inequality, asserted on its own)."""
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    for direction in DIRECTIONS:
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        ai, pi, li = _t(a), _t(c["p"]), _t(lab)
        _, lse = eng.ce_f32_fwd(T, direction, ai, pi, li)
        g = _t(c["g_rows"])
        want_e, want_r = c[f"grad64_{direction}_rows"]
        ce, cr = _table_grads(c, direction, *_composed(eng, T, c, direction, g, n))
        bound_e, bound_r = 4 * max(_err(ce, want_e), EPS), 4 * max(_err(cr, want_r), EPS)
        runs = {}
        for cc in (128, 256, 0):
            runs[cc] = eng.ce_f32_bwd(T, direction, ai, pi, li, lse, g_rows=g, chunk_cols=cc)
            again = eng.ce_f32_bwd(T, direction, ai, pi, li, lse, g_rows=g, chunk_cols=cc)
            for nm, x, y in zip(("g_a", "g_p", "g_tgt"), runs[cc], again):
                assert torch.equal(x, y), f"{nm}: two runs of chunk_cols {cc} differ"
            fe, fr = _table_grads(c, direction, *runs[cc])
            ee, er = _err(fe, want_e), _err(fr, want_r)
            print(f"CHUNK {name} d{d} E{E} {direction} chunk {cc}: entity {ee:.3e} (bound {bound_e:.3e}) relation {er:.3e} "
                  f"(bound {bound_r:.3e})")
            assert ee <= bound_e and er <= bound_r, (cc, ee, bound_e, er, bound_r)
        one_e, one_r = _table_grads(c, direction, *runs[0])
        for cc in (128, 256):
            assert torch.equal(runs[cc][2], runs[0][2]), f"g_tgt differs between chunk_cols {cc} and one chunk"
            fe, fr = _table_grads(c, direction, *runs[cc])
            de, dr = _err(fe, one_e), _err(fr, one_r)
            print(f"CHUNK {name} d{d} E{E} {direction} chunk {cc} vs one chunk: entity {de:.3e} relation {dr:.3e}")
            assert de <= 2 * bound_e and dr <= 2 * bound_r, (cc, de, dr)


@pytest.mark.parametrize("name,d,E,R,n,ld", [("complex", 16, 150, 5, 37, 16), ("distmult", 40, 128 * 17 + 1, 5, 130, 48),
                                            ("complex", 8, 129, 3, 1, 8)])
def test_guards_and_workspace_tail_are_untouched(eng, name, d, E, R, n, ld):
    from kge_amd import _lib
    from kge_amd._lib import PO_, SP_
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    lib, tc = _lib.lib(), T.c()
    for direction, cc in (("sp", 0), ("po", 128)):
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        keep = []
        ai, pi, li = (eng._index(x, T.device, keep) for x in (_t(a), _t(c["p"]), _t(lab)))
        need = lib.kge_ce_f32_workspace_bytes(ctypes.byref(tc), n, cc)
        assert need > 0 and need % 256 == 0
        S = 7.25  # sentinel
        ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        rows = torch.full((2, n + 2), S, device=DEV)
        ga, gp, gt = (torch.full((r + 2, d), S, device=DEV) for r in (n, n, E))
        st = eng._stream(T.device)
        dirc = SP_ if direction == "sp" else PO_
        g = _t(c["g_rows"])
        _lib.check(lib.kge_ce_f32_fwd(ctypes.byref(tc), dirc, ai, pi, li, n, rows[0, 1:].data_ptr(), rows[1, 1:].data_ptr(),
                                      ws.data_ptr(), need, st), "fwd")
        _lib.check(lib.kge_ce_f32_bwd(ctypes.byref(tc), dirc, ai, pi, li, n, rows[1, 1:].data_ptr(), g.data_ptr(), 1.0,
                                      ga[1:].data_ptr(), gp[1:].data_ptr(), gt[1:].data_ptr(), ws.data_ptr(), need, st), "bwd")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0x5A).all()), "workspace tail written"
        assert bool((rows[:, 0] == S).all()) and bool((rows[:, n + 1] == S).all()), "loss_rows / lse guards"
        for nm, x, r in (("g_a", ga, n), ("g_p", gp, n), ("g_tgt", gt, E)):
            assert bool((x[0] == S).all()) and bool((x[r + 1] == S).all()), nm + " guard rows"
            assert bool(torch.isfinite(x[1:r + 1]).all()) and not bool((x[1:r + 1] == S).any()), nm
        want = eng.ce_f32_bwd(T, direction, _t(a), _t(c["p"]), _t(lab), rows[1, 1:n + 1].contiguous(), g_rows=g, chunk_cols=cc)
        for x, w, r in zip((ga, gp, gt), want, (n, n, E)):
            assert torch.equal(x[1:r + 1], w)
        # too small a workspace is refused
        assert lib.kge_ce_f32_bwd(ctypes.byref(tc), dirc, ai, pi, li, n, rows[1, 1:].data_ptr(), g.data_ptr(), 1.0,
                                  ga[1:].data_ptr(), gp[1:].data_ptr(), gt[1:].data_ptr(), ws.data_ptr(), 256, st) == -5


def test_int32_repeats_empty_and_bad_label(eng):
    name, d, E, R, n, ld = "complex", 16, 150, 5, 37, 16
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    tri = np.stack([c["s"], c["p"], c["o"]], 1)
    t32 = _t(tri.astype(np.int32))
    loss, lse = eng.ce_f32_fwd(T, "sp", t32[:, 0], t32[:, 1], t32[:, 2])
    loss64, lse64 = eng.ce_f32_fwd(T, "sp", _t(tri[:, 0]), _t(tri[:, 1]), _t(tri[:, 2]))
    assert torch.equal(loss, loss64) and torch.equal(lse, lse64)
    e = torch.zeros(0, dtype=torch.int64, device=DEV)
    l0, s0 = eng.ce_f32_fwd(T, "po", e, e, e)
    assert l0.shape == (0,) and s0.shape == (0,)
    g0 = eng.ce_f32_bwd(T, "po", e, e, e, s0)
    assert g0[0].shape == (0, d) and g0[2].shape == (E, d) and float(g0[2].abs().max()) == 0.0
    bad = tri[:, 2].copy()
    bad[3], bad[11] = E, -1
    lb, sb = eng.ce_f32_fwd(T, "sp", _t(tri[:, 0]), _t(tri[:, 1]), _t(bad))
    nan = torch.isnan(lb).cpu().numpy()
    assert nan.tolist() == [i in (3, 11) for i in range(n)]
    assert torch.equal(sb, lse64)


def test_unsupported_tables_are_refused(eng):
    from kge_amd import _lib
    from kge_amd import model as km
    ix = torch.zeros(4, dtype=torch.int64, device=DEV)
    for name, d, dt in (("complex", 36, torch.float32), ("complex", 64, torch.bfloat16), ("distmult", 64, torch.bfloat16)):
        T = eng.Tables(name, torch.randn(70, d, device=DEV).to(dt), torch.randn(3, d, device=DEV).to(dt))
        assert not eng.ce_f32_supported(T)
        with pytest.raises(RuntimeError):
            eng.ce_f32_fwd(T, "sp", ix, ix, ix)
        keep = []
        a = eng._index(ix, T.device, keep)
        buf = torch.zeros(1 << 16, device=DEV)
        P = buf.data_ptr()
        assert _lib.lib().kge_ce_f32_fwd(ctypes.byref(T.c()), 1, a, a, a, 4, P, P, P, 1 << 18, None) == -2
        assert _lib.lib().kge_ce_f32_bwd(ctypes.byref(T.c()), 1, a, a, a, 4, P, None, 1.0, P, P, P, P, 1 << 18, None) == -2
    assert eng.ce_f32_supported(eng.Tables("distmult", torch.randn(70, 64, device=DEV), torch.randn(3, 64, device=DEV)))
    assert not eng.ce_f32_supported(eng.Tables("transe", torch.randn(70, 64, device=DEV), torch.randn(3, 64, device=DEV)))
    # kge_amd.model: no fused tables, so loss_sp composes the loss (the plugin's models return None instead:
    # tests/test_gpu_libkge_plugin_ce_f32.py::test_unsupported_configurations_return_none)
    for kw in ({"dim": 36}, {"dim": 64, "dtype": torch.bfloat16}):
        m = km.create("complex", 70, 3, kw["dim"], device=DEV, dtype=kw.get("dtype", torch.float32), fused_f32_loss=True)
        assert m._ce_f32_tables() is None


def test_memory_bound_of_a_model_step():
    """n = 256, E = 131,072, d = 16: one [n, E] float32 matrix is 128 MB (the composed path holds several).  The fused
    step raises max_memory_allocated by less than 64 MB over what is held after a warm-up step (the bound of
    tests/test_gpu_ce_dist.py::test_memory_bound_of_a_model_step)."""
    from kge_amd import model as km
    E, R, d, n = 131072, 7, 16, 256
    torch.manual_seed(0)
    m = km.create("complex", E, R, d, device=DEV, fused_f32_loss=True).train()
    assert m._ce_f32_tables() is not None
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


@pytest.mark.parametrize("name", ["complex", "distmult"])
def test_model_level_one_sgd_step_fused_against_composed(name):
    """km.create(..., fused_f32_loss=True) against fused_f32_loss=False from identical parameters: the loss and the
    parameters after one SGD step, each within 4 x the composed model's own error against the float64 step."""
    from kge_amd import model as km
    E, R, d, n, lr = 3005, 11, 64, 300, 0.5
    g = torch.Generator().manual_seed(2)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    res = {}
    for fused in (True, False):
        torch.manual_seed(0)
        m = km.create(name, E, R, d, device=DEV, fused_f32_loss=fused).train()
        assert (m._ce_f32_tables() is not None) == fused
        we, wr = m.get_s_embedder().weight, m.get_p_embedder().weight
        if fused:
            e64, r64 = we.detach().double().cpu().requires_grad_(), wr.detach().double().cpu().requires_grad_()
        opt = torch.optim.SGD(m.parameters(), lr=lr)
        total = m.loss_sp_po(s, p, o).sum() / n
        total.backward()
        opt.step()
        res[fused] = (float(total), we.detach().double().cpu(), wr.detach().double().cpu())
    sc, pc, oc = s.cpu(), p.cpu(), o.cpu()
    ce = torch.nn.functional.cross_entropy
    t64 = (ce(tp.score_sp(name, e64, r64, sc, pc), oc, reduction="sum") + ce(tp.score_po(name, e64, r64, pc, oc), sc, reduction="sum")) / n
    t64.backward()
    want = (float(t64), (e64 - lr * e64.grad).detach(), (r64 - lr * r64.grad).detach())
    (lf, ef, rf), (lc, ec, rc) = res[True], res[False]
    for nm, f, cm, w in (("loss", lf, lc, want[0]), ("entity", ef, ec, want[1]), ("relation", rf, rc, want[2])):
        errf, errc = (abs(f - w), abs(cm - w)) if nm == "loss" else (float((f - w).abs().max()), float((cm - w).abs().max()))
        print(f"MODEL {name} {nm}: vs float64 fused {errf:.3e} composed {errc:.3e}")
        assert errf <= 4 * max(errc, EPS * max(1.0, abs(w) if nm == "loss" else float(w.abs().max()))), (nm, errf, errc)
