"""KvsAll kl and bce losses of ComplEx / DistMult on FLOAT32 tables without a score matrix (kge_kl_f32_* / kge_bce_f32_*,
ce_f32.hip) on the MI355X: the forward against float64 and against the same formulas on the project's own stored scores
and the oracle's, lse bit for bit against kge_ce_f32_fwd, two runs bit for bit, the backward against float64 autograd
and against the composed device path (score_sp -> KgeModel._kl_composed / _bce_composed in float32 -> autograd ->
kge_score_pairs_bwd), chunkings against each other, guards and the label bits, bad labels, unsupported tables, the model
with its memory bound.  Shapes, tables and queries are those of test_gpu_ce_f32.py.

The backward's bound is that of test_gpu_ce_f32.py: per case the COMPOSED path's own max-abs error against float64 is
measured and the fused path is allowed 4 x that (floor 2^-24).  Measured on an MI355X over the 240 comparisons of
test_backward_against_float64_autograd_and_the_composed_path (max |err| / max(1, |want|max), entity and relation table
gradients; kl and bce with row and scalar upstream gradient, weighted kl with label_bias): composed 4.91e-9 .. 8.99e-7,
fused at most 8.80e-7, fused / max(composed, 2^-24) at most 3.17 (the weighted kl with label_bias at E = 38,401; kl 2.86,
bce 1.62).  The composed path's own error -- kge_score_pairs_bwd on float32 tables, the yardstick
here -- is asserted against a derived rounding bound in tests/test_gpu_pairs_bwd.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import torch_port as tp
import test_gpu_ce_f32 as ce32
import _multilabel_f32_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES, WALK = ce32.SHAPES, ce32.WALK
CASES = [(name, *shape) for shape in SHAPES + [WALK] for name in ("complex", "distmult")]
DIRECTIONS = ce32.DIRECTIONS
OFFSET = 3.0
EPS = ce32.EPS
_t, _tables, _table_grads, _err = ce32._t, ce32._tables, ce32._table_grads, ce32._err


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _label_weight(n):
    return np.random.default_rng(6).uniform(0.05, 1.0, n).astype(np.float32)


def _label_bias(n, E):
    return (np.random.default_rng(7).uniform(0.2, 1.0, n) / E).astype(np.float32)


def _rows64(kind, sc, y, k, w, b):
    """float64 torch loss rows on scores sc [n, E] with dense labels y: kl, bce (offset 3), klw (weight and bias)"""
    if kind == "kl":
        kk = k.clamp_min(1.0)
        rows = torch.logsumexp(sc, 1) - (sc * y).sum(1) / kk - torch.log(kk)
        return torch.where(k > 0, rows, torch.zeros_like(rows))
    if kind == "bce":
        return tp.bce_loss(sc, y, OFFSET, reduction="rows")
    return torch.logsumexp(sc, 1) - w * (sc * y).sum(1) - b * sc.sum(1)


GRADS = (("kl", "rows"), ("kl", "scalar"), ("bce", "rows"), ("bce", "scalar"), ("klw", "rows"))


@functools.lru_cache(maxsize=None)
def _case(name, d, E, R, n, ld):
    """test_gpu_ce_f32's case (tables, queries, oracle scores, g_rows) + label sets per direction + the float64 autograd
    gradients of the losses: computed once and shared, never modified."""
    c = dict(ce32._case(name, d, E, R, n, ld))
    rng = np.random.default_rng(17 + 1000 * d + n)
    w64 = torch.from_numpy(_label_weight(n).astype(np.float64))
    b64 = torch.from_numpy(_label_bias(n, E).astype(np.float64))
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        rowptr, col = ref.labels(rng, n, E)
        c["csr_" + direction] = (rowptr, col)
        y = torch.from_numpy(ref.dense(rowptr, col, n, E))
        k = torch.from_numpy(np.diff(rowptr).astype(np.float64))
        e64 = torch.from_numpy(c["ent"]).double().requires_grad_()
        r64 = torch.from_numpy(c["rel"]).double().requires_grad_()
        ai, pi = torch.from_numpy(a), torch.from_numpy(c["p"])
        sc = tp.score_sp(name, e64, r64, ai, pi) if direction == "sp" else tp.score_po(name, e64, r64, pi, ai)
        for kind, gname in GRADS:
            g = c["g_rows"].astype(np.float64) if gname == "rows" else np.full(n, np.float64(np.float32(0.37)))
            rows = _rows64(kind, sc, y, k, w64, b64)
            ge, gr = torch.autograd.grad((rows * torch.from_numpy(g)).sum(), (e64, r64), retain_graph=True)
            c[f"grad64_{kind}_{direction}_{gname}"] = (ge.numpy(), gr.numpy())
        c["sc64_" + direction] = sc.detach().numpy()
    return c


def test_label_sets_cover_what_they_should():
    counts, all_entities, shuffled = set(), False, 0
    for d, E, R, n, ld in SHAPES + [WALK]:
        rowptr, col = ref.labels(np.random.default_rng(17 + 1000 * d + n), n, E)
        k = np.diff(rowptr)
        rows = [col[rowptr[i]:rowptr[i + 1]] for i in range(n)]
        assert all(len(set(r.tolist())) == len(r) for r in rows), "ids unique per row"
        assert col.min() >= 0 and col.max() < E
        counts |= set(k.tolist())
        seen = set(col.tolist())
        assert set(ref.edge_columns(E)) <= seen, (E, sorted(set(ref.edge_columns(E)) - seen))
        assert {0, E - 1} <= seen
        if E > 128:
            assert {127, 128} <= seen and (E - 1) // 128 * 128 - 121 in seen   # a tile edge, the last tile but one
        if E > 32:
            assert {31, 32} <= seen                                            # a mask word's edge
        if E == 129:
            all_entities = any(len(r) == E for r in rows)
        shuffled += sum(len(r) > 1 and not np.array_equal(r, np.sort(r)) for r in rows)
        if n >= 7:
            assert k[:6].tolist() == [0, 1, 2, 63, 64, 65] and k[6] == min(130, E)
    assert {0, 1, 2, 63, 64, 65} <= counts and max(counts) > 128
    assert all_entities, "one row labelled with every entity at E = 129"
    assert shuffled > 100


def _fwd(eng, kind, T, direction, ai, pi, csr, label_weight=None, **kw):
    """(loss_rows, lse or None)"""
    if kind == "kl":
        return eng.kl_f32_fwd(T, direction, ai, pi, csr[0], csr[1], label_weight, **kw)
    return eng.bce_f32_fwd(T, direction, ai, pi, csr[0], csr[1], OFFSET, **kw), None


def _bwd(eng, kind, T, direction, ai, pi, csr, lse, **kw):
    if kind == "kl":
        return eng.kl_f32_bwd(T, direction, ai, pi, csr[0], csr[1], lse, **kw)
    return eng.bce_f32_bwd(T, direction, ai, pi, csr[0], csr[1], OFFSET, **kw)


@pytest.mark.parametrize("name,d,E,R,n,ld", CASES)
def test_forward_lse_bits_and_determinism(eng, name, d, E, R, n, ld):
    """loss_rows / lse of kl (unweighted, weighted) and bce (offset 3) against float64 scores, against the formulas on
    the stored float32 scores and on the oracle's; lse BIT-equal to kge_ce_f32_fwd's; two runs bit-equal."""
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    assert eng.multilabel_f32_supported(T)
    w = _label_weight(n)
    for direction in DIRECTIONS:
        a, lab = (c["s"], c["o"]) if direction == "sp" else (c["o"], c["s"])
        ai, pi = _t(a), _t(c["p"])
        rowptr, col = c["csr_" + direction]
        csr, k = (_t(rowptr), _t(col)), np.diff(rowptr)
        sc = (eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)).cpu().numpy()
        assert np.array_equal(sc, c["oracle_" + direction]), "stored scores differ from the oracle's"
        _, lse_ce = eng.ce_f32_fwd(T, direction, ai, pi, _t(lab))
        for kind, lw in (("kl", None), ("kl", w), ("bce", None)):
            lwt = None if lw is None else _t(lw)
            loss, lse = _fwd(eng, kind, T, direction, ai, pi, csr, lwt)
            loss2, lse2 = _fwd(eng, kind, T, direction, ai, pi, csr, lwt)
            assert torch.equal(loss, loss2) and (lse is None or torch.equal(lse, lse2)), "two runs differ"
            if lse is not None:
                assert torch.equal(lse, lse_ce), "lse differs from kge_ce_f32_fwd's"
            got = {"loss": loss.cpu().numpy().astype(np.float64)}
            if lse is not None:
                got["lse"] = lse.cpu().numpy().astype(np.float64)
            assert all(np.isfinite(v).all() for v in got.values()), (kind, direction)
            for ref_name, x in (("float64", c["sc64_" + direction]), ("stored", sc), ("oracle", c["oracle_" + direction])):
                if kind == "kl":
                    want_loss, want_lse = ref.kl_rows(x, rowptr, col, lw)
                else:
                    want_loss, want_lse = ref.bce_rows(x, rowptr, col, OFFSET), None
                for nm, g, want in (("loss", got["loss"], want_loss), ("lse", got.get("lse"), want_lse)):
                    if g is None:
                        continue
                    err, tol = np.abs(g - want), 1e-5 + 1e-5 * np.abs(want)   # (tests/test_gpu_multilabel_dist.py's bound)
                    print(f"FWD {name} d{d} E{E} {direction} {kind} weight {lw is not None} {nm} vs {ref_name}: "
                          f"max err {err.max():.3e} min tol {tol.min():.3e}")
                    assert (err <= tol).all(), (kind, direction, ref_name, nm, float(err.max()), int((err > tol).sum()))
            if kind == "kl" and lw is None:
                assert (got["loss"][k == 0] == 0.0).all(), "kl: a row without labels has loss 0"
            if kind == "kl" and lw is not None:
                assert np.array_equal(got["loss"][k == 0], got["lse"][k == 0]), "weighted kl: a row without labels has lse"


def _composed(eng, km, T, c, kind, direction, g, n, E, w=None, b=None):
    """The composed device path: score_sp / score_po -> the model's composed float32 loss -> autograd ->
    kge_score_pairs_bwd"""
    a = c["s"] if direction == "sp" else c["o"]
    ai, pi = _t(a), _t(c["p"])
    rowptr, col = (_t(x) for x in c["csr_" + direction])
    sc = (eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)).clone().requires_grad_()
    if kind == "kl":
        rows = km.KgeModel._kl_composed(sc, rowptr, col)
    elif kind == "bce":
        rows = km.KgeModel._bce_composed(sc, rowptr, col, OFFSET)
    else:  # the weighted loss with its bias term, from the same float32 ops
        y = torch.zeros_like(sc)
        y[torch.repeat_interleave(torch.arange(n, device=DEV), rowptr[1:] - rowptr[:-1]), col] = 1.0
        rows = torch.logsumexp(sc, 1) - w * (sc * y).sum(1) - b * sc.sum(1)
    (rows * g).sum().backward()
    return eng.score_pairs_bwd(T, direction, ai, pi, None, sc.grad.contiguous(), sc.detach())


@pytest.mark.parametrize("name,d,E,R,n,ld", CASES)
def test_backward_against_float64_autograd_and_the_composed_path(eng, name, d, E, R, n, ld):
    from kge_amd import model as km
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    w, b = _t(_label_weight(n)), _t(_label_bias(n, E))
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        ai, pi = _t(a), _t(c["p"])
        csr = tuple(_t(x) for x in c["csr_" + direction])
        lse = eng.kl_f32_fwd(T, direction, ai, pi, *csr)[1]
        for kind, gname in GRADS:
            kw, g = (({"g_rows": _t(c["g_rows"])}, _t(c["g_rows"])) if gname == "rows"
                     else ({"g_scalar": 0.37}, torch.full((n,), 0.37, device=DEV)))
            if kind == "klw":
                kw = dict(kw, label_weight=w, label_bias=b)
            want_e, want_r = c[f"grad64_{kind}_{direction}_{gname}"]
            fe, fr = _table_grads(c, direction, *_bwd(eng, "bce" if kind == "bce" else "kl", T, direction, ai, pi, csr, lse, **kw))
            ce, cr = _table_grads(c, direction, *_composed(eng, km, T, c, kind, direction, g, n, E, w, b))
            for nm, f, cm, wnt in (("entity", fe, ce, want_e), ("relation", fr, cr, want_r)):
                ef, ec, efc = _err(f, wnt), _err(cm, wnt), _err(f, cm)
                print(f"BWD {name} d{d} E{E} n{n} {kind} {direction} {gname} {nm}: vs float64 fused {ef:.3e} composed "
                      f"{ec:.3e} bound {4 * max(ec, EPS):.3e}; fused vs composed {efc:.3e}")
                bound = 4 * max(ec, EPS)
                assert ef <= bound, (kind, nm, ef, ec)
                assert efc <= bound + ec, (kind, nm, efc, ec)   # (triangle: both within their bound of float64)


@pytest.mark.parametrize("name", ["complex", "distmult"])
@pytest.mark.parametrize("d,E,R,n,ld", [(128, 1037, 13, 203, 128), (40, 128 * 17 + 1, 5, 130, 48)])
def test_chunkings_agree(eng, name, d, E, R, n, ld):
    """chunk_cols 128, 256 and 0 (here: one chunk): g_tgt BIT-equal across the three, every output bit-equal across two
    runs of one chunking; g_a / g_p as test_gpu_ce_f32.py::test_chunkings_agree asserts them: the table gradients of EACH
    chunking within the backward's bound of float64 (4 x the composed path's error) and of each chunked run within
    twice that bound of the one-chunk run."""
    from kge_amd import model as km
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    w, b = _t(_label_weight(n)), _t(_label_bias(n, E))
    g = _t(c["g_rows"])
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        ai, pi = _t(a), _t(c["p"])
        csr = tuple(_t(x) for x in c["csr_" + direction])
        lse = eng.kl_f32_fwd(T, direction, ai, pi, *csr)[1]
        for kind, extra in (("kl", {}), ("klw", {"label_weight": w, "label_bias": b}), ("bce", {})):
            want_e, want_r = c[f"grad64_{kind}_{direction}_rows"]
            ce, cr = _table_grads(c, direction, *_composed(eng, km, T, c, kind, direction, g, n, E, w, b))
            bound_e, bound_r = 4 * max(_err(ce, want_e), EPS), 4 * max(_err(cr, want_r), EPS)
            runs = {}
            for cc in (128, 256, 0):
                call = lambda: _bwd(eng, "bce" if kind == "bce" else "kl", T, direction, ai, pi, csr, lse, g_rows=g,
                                    chunk_cols=cc, **extra)
                runs[cc] = call()
                for nm, x, y in zip(("g_a", "g_p", "g_tgt"), runs[cc], call()):
                    assert torch.equal(x, y), f"{nm}: two runs of chunk_cols {cc} differ"
                fe, fr = _table_grads(c, direction, *runs[cc])
                ee, er = _err(fe, want_e), _err(fr, want_r)
                print(f"CHUNK {name} d{d} E{E} {kind} {direction} chunk {cc}: entity {ee:.3e} (bound {bound_e:.3e}) "
                      f"relation {er:.3e} (bound {bound_r:.3e})")
                assert ee <= bound_e and er <= bound_r, (kind, cc, ee, bound_e, er, bound_r)
            one_e, one_r = _table_grads(c, direction, *runs[0])
            for cc in (128, 256):
                assert torch.equal(runs[cc][2], runs[0][2]), f"g_tgt differs between chunk_cols {cc} and one chunk"
                fe, fr = _table_grads(c, direction, *runs[cc])
                de, dr = _err(fe, one_e), _err(fr, one_r)
                assert de <= 2 * bound_e and dr <= 2 * bound_r, (kind, cc, de, dr)


def _layout(T, n, E, ws_bytes):
    """(C, byte offset of the label bits, the forward's minimum) as include/kge_amd.h lays the workspace out: kge_ce_f32's
    fixed part | G [n, C] | n C / 8 bytes of bits, each on 256 bytes; C the largest multiple of 128 that fits, at most E
    rounded up."""
    from kge_amd import _lib
    al = lambda x: -(-x // 256) * 256
    d = T.ent.shape[1]
    head = _lib.lib().kge_ce_f32_workspace_bytes(ctypes.byref(T.c()), n, 128) - al(4 * n * 128)
    left = ws_bytes - head
    C = min(left // n * 8 // 33 // 128 * 128, -(-E // 128) * 128)
    while C >= 128 and al(4 * n * C) + al(n * C // 8) > left:
        C -= 128
    fwd_min = head - al(min(32, max(1, (8 << 20) // (4 * n * d))) * 4 * n * d)   # records + the two [n, d] buffers
    return C, head + al(4 * n * C), fwd_min


@pytest.mark.parametrize("kind", ["kl", "bce"])
@pytest.mark.parametrize("name,d,E,R,n,ld", [("complex", 16, 150, 5, 37, 16), ("distmult", 40, 128 * 17 + 1, 5, 130, 48),
                                            ("complex", 8, 129, 3, 1, 8)])
def test_guards_workspace_tail_and_the_label_bits(eng, kind, name, d, E, R, n, ld):
    """Sentinels behind and in front of loss_rows, lse, g_a, g_p and g_tgt (rows >= n among them) and the workspace
    behind the computed size stay untouched; the label bits -- zero before -- are zero after the backward; the raw
    calls give the engine's bits; workspaces below the documented minima are refused."""
    from kge_amd import _lib
    from kge_amd._lib import PO_, SP_
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    lib, tc = _lib.lib(), T.c()
    g = _t(c["g_rows"])
    for direction, cc in (("sp", 0), ("po", 128)):
        a = c["s"] if direction == "sp" else c["o"]
        csr = tuple(_t(x) for x in c["csr_" + direction])
        rp, cl = csr[0].data_ptr(), csr[1].data_ptr()
        keep = []
        ai, pi = (eng._index(x, T.device, keep) for x in (_t(a), _t(c["p"])))
        need = lib.kge_multilabel_f32_workspace_bytes(ctypes.byref(tc), n, cc)
        assert need > 0 and need % 256 == 0
        C, mask0, fwd_min = _layout(T, n, E, need)
        assert C >= (cc or 128) and C % 128 == 0 and mask0 + n * C // 8 <= need
        S = float("nan")  # canary
        ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        ws[mask0:mask0 + n * C // 8] = 0
        rows = torch.full((2, n + 2), S, device=DEV)
        ga, gp, gt = (torch.full((r + 2, d), S, device=DEV) for r in (n, n, E))
        st = eng._stream(T.device)
        dirc = SP_ if direction == "sp" else PO_
        if kind == "kl":
            fwd = lambda w, wb: lib.kge_kl_f32_fwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, None, rows[0, 1:].data_ptr(),
                                                   rows[1, 1:].data_ptr(), w, wb, st)
            bwd = lambda w, wb: lib.kge_kl_f32_bwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, None, None,
                                                   rows[1, 1:].data_ptr(), g.data_ptr(), 1.0, ga[1:].data_ptr(),
                                                   gp[1:].data_ptr(), gt[1:].data_ptr(), w, wb, st)
        else:
            fwd = lambda w, wb: lib.kge_bce_f32_fwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, OFFSET,
                                                    rows[0, 1:].data_ptr(), w, wb, st)
            bwd = lambda w, wb: lib.kge_bce_f32_bwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, OFFSET, g.data_ptr(), 1.0,
                                                    ga[1:].data_ptr(), gp[1:].data_ptr(), gt[1:].data_ptr(), w, wb, st)
        # below the documented minima: refused, nothing written
        assert fwd(ws.data_ptr(), fwd_min - 256) == -5
        assert bwd(ws.data_ptr(), lib.kge_multilabel_f32_workspace_bytes(ctypes.byref(tc), n, 128) - 256) == -5
        torch.cuda.synchronize()
        assert bool(torch.isnan(rows).all()) and all(bool(torch.isnan(x).all()) for x in (ga, gp, gt))
        _lib.check(fwd(ws.data_ptr(), fwd_min), "fwd")   # the forward's minimum is enough
        _lib.check(bwd(ws.data_ptr(), need), "bwd")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0x5A).all()), "workspace tail written"
        assert bool((ws[mask0:mask0 + n * C // 8] == 0).all()), "label bits not left zero"
        assert bool((ws[mask0 + n * C // 8:need] == 0x5A).all()), "padding behind the label bits written"
        assert bool(torch.isnan(rows[0, 0])) and bool(torch.isnan(rows[:, n + 1]).all()), "loss_rows / lse guards"
        assert bool(torch.isfinite(rows[0, 1:n + 1]).all())
        if kind == "bce":
            assert bool(torch.isnan(rows[1]).all()), "bce writes no lse"
        else:
            assert bool(torch.isnan(rows[1, 0])) and bool(torch.isfinite(rows[1, 1:n + 1]).all())
        for nm, x, r in (("g_a", ga, n), ("g_p", gp, n), ("g_tgt", gt, E)):
            assert bool(torch.isnan(x[0]).all()) and bool(torch.isnan(x[r + 1]).all()), nm + " guard rows"
            assert bool(torch.isfinite(x[1:r + 1]).all()), nm + ": not written"
        loss, lse = _fwd(eng, kind, T, direction, _t(a), _t(c["p"]), csr, chunk_cols=cc)
        assert torch.equal(rows[0, 1:n + 1], loss) and (lse is None or torch.equal(rows[1, 1:n + 1], lse))
        want = _bwd(eng, kind, T, direction, _t(a), _t(c["p"]), csr, lse, g_rows=g, chunk_cols=cc)
        for x, wnt, r in zip((ga, gp, gt), want, (n, n, E)):
            assert torch.equal(x[1:r + 1], wnt)


def test_int32_strided_empty_and_bad_labels(eng):
    """int32 and strided query indices and an int32 CSR give the int64 bits; n = 0 zero-fills g_tgt; labels -1 and E make
    their rows NaN and leave every other row and lse bit-equal to the call without them; the backward ignores them: it
    equals the backward with the bad labels removed (for the unweighted kl loss with the weights 1 / k_i of the CSR
    that was passed, since k_i counts what the CSR holds)."""
    name, d, E, R, n, ld = "complex", 16, 150, 5, 37, 16
    c = _case(name, d, E, R, n, ld)
    T = _tables(eng, name, c, ld)
    rowptr, col = c["csr_sp"]
    csr = (_t(rowptr), _t(col))
    tri = np.stack([c["s"], c["p"], c["o"]], 1)
    t32, t64 = _t(tri.astype(np.int32)), _t(tri)
    g = _t(c["g_rows"])
    a64, p64 = t64[:, 0].contiguous(), t64[:, 1].contiguous()
    # the CSR with two more entries: E in row 4 (third place), -1 in front of row 9
    ins = [int(rowptr[4] + 2), int(rowptr[9])]
    bad_col = np.insert(col, ins, [E, -1])
    bad_rowptr = rowptr.copy()
    bad_rowptr[5:] += 1
    bad_rowptr[10:] += 1
    bad = (_t(bad_rowptr), _t(bad_col))
    for kind in ("kl", "bce"):
        loss, lse = _fwd(eng, kind, T, "sp", t32[:, 0], t32[:, 1], (csr[0].int(), csr[1].int()))
        loss64, lse64 = _fwd(eng, kind, T, "sp", a64, p64, csr)
        assert torch.equal(loss, loss64) and (lse is None or torch.equal(lse, lse64))
        g32 = _bwd(eng, kind, T, "sp", t32[:, 0], t32[:, 1], csr, lse, g_rows=g)
        g64 = _bwd(eng, kind, T, "sp", a64, p64, csr, lse64, g_rows=g)
        assert all(torch.equal(x, y) for x, y in zip(g32, g64))
        # n = 0
        e, rp0 = torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        l0, s0 = _fwd(eng, kind, T, "po", e, e, (rp0, e))
        assert l0.shape == (0,) and (s0 is None or s0.shape == (0,))
        g0 = _bwd(eng, kind, T, "po", e, e, (rp0, e), s0)
        assert g0[0].shape == (0, d) and g0[1].shape == (0, d) and g0[2].shape == (E, d)
        assert float(g0[2].abs().max()) == 0.0
        # (the C entry itself zero-fills g_tgt for n = 0, as run_ce_f32_bwd does)
        from kge_amd import _lib
        gt = torch.full((E, d), float("nan"), device=DEV)
        nul = _lib.KgeIndex(None, 1, 0, 1)
        lib, tc, st = _lib.lib(), T.c(), eng._stream(T.device)
        if kind == "kl":
            rc = lib.kge_kl_f32_bwd(ctypes.byref(tc), 1, nul, nul, 0, None, None, None, None, None, None, 1.0, None, None,
                                    gt.data_ptr(), None, 0, st)
        else:
            rc = lib.kge_bce_f32_bwd(ctypes.byref(tc), 1, nul, nul, 0, None, None, 0.0, None, 1.0, None, None,
                                     gt.data_ptr(), None, 0, st)
        torch.cuda.synchronize()
        assert rc == 0 and float(gt.abs().max()) == 0.0
        # labels out of range
        for lw in ((None, _t(_label_weight(n))) if kind == "kl" else (None,)):
            good_l, good_s = _fwd(eng, kind, T, "sp", a64, p64, csr, lw)
            lb, sb = _fwd(eng, kind, T, "sp", a64, p64, bad, lw)
            nan = torch.isnan(lb).cpu().numpy()
            assert nan.tolist() == [i in (4, 9) for i in range(n)]
            assert sb is None or torch.equal(sb, good_s)
            keep = torch.from_numpy(~nan).to(DEV)
            assert torch.equal(lb[keep], good_l[keep])
            kw = {} if kind == "bce" else {"label_weight": lw}
            gb = _bwd(eng, kind, T, "sp", a64, p64, bad, good_s, g_rows=g, **kw)
            if kind == "kl" and lw is None:   # the weights the bad CSR implies, on the good CSR
                kw = {"label_weight": _t((1.0 / np.diff(bad_rowptr).clip(1)).astype(np.float32)),
                      "g_rows": torch.where(_t(np.diff(bad_rowptr)) > 0, g, torch.zeros_like(g))}
            else:
                kw = dict(kw, g_rows=g)
            gg = _bwd(eng, kind, T, "sp", a64, p64, csr, good_s, **kw)
            assert all(bool(torch.isfinite(x).all()) for x in gb)
            assert all(torch.equal(x, y) for x, y in zip(gb, gg)), (kind, lw is not None)


def test_unsupported_tables_are_refused(eng):
    from kge_amd import _lib
    lib = _lib.lib()
    ix = torch.zeros(4, dtype=torch.int64, device=DEV)
    rp, cl = torch.arange(5, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    ent, rel = torch.randn(70, 64, device=DEV), torch.randn(3, 64, device=DEV)
    wide = torch.randn(70, 65, device=DEV)[:, 1:]       # rows off 16 bytes (base and pitch)
    tables = [eng.Tables("complex", ent.bfloat16(), rel.bfloat16()), eng.Tables("distmult", ent.bfloat16(), rel.bfloat16()),
              eng.Tables("transe", ent, rel), eng.Tables("complex", ent[:, :12].contiguous(), rel[:, :12].contiguous()),
              eng.Tables("distmult", wide, rel)]
    for T in tables:
        assert lib.kge_multilabel_f32_workspace_bytes(ctypes.byref(T.c()), 4, 0) == 0
        assert not eng.multilabel_f32_supported(T)
        with pytest.raises(RuntimeError):
            eng.kl_f32_fwd(T, "sp", ix, ix, rp, cl)
        with pytest.raises(RuntimeError):
            eng.bce_f32_bwd(T, "sp", ix, ix, rp, cl)
        # the C entries themselves: refused with nothing written
        keep, out = [], torch.full((3, 8), 7.25, device=DEV)
        ai = eng._index(ix, T.device, keep)
        ws = torch.full((1 << 18,), 0x5A, dtype=torch.uint8, device=DEV)
        P, tc, st = ws.data_ptr(), T.c(), eng._stream(T.device)
        o = [out[i].data_ptr() for i in range(3)]
        assert lib.kge_kl_f32_fwd(ctypes.byref(tc), 1, ai, ai, 4, rp.data_ptr(), cl.data_ptr(), None, o[0], o[1], P, 1 << 18, st) == -2
        assert lib.kge_bce_f32_fwd(ctypes.byref(tc), 1, ai, ai, 4, rp.data_ptr(), cl.data_ptr(), 0.0, o[2], P, 1 << 18, st) == -2
        assert lib.kge_kl_f32_bwd(ctypes.byref(tc), 1, ai, ai, 4, rp.data_ptr(), cl.data_ptr(), None, None, o[1], None, 1.0,
                                  o[0], o[0], o[0], P, 1 << 18, st) == -2
        assert lib.kge_bce_f32_bwd(ctypes.byref(tc), 1, ai, ai, 4, rp.data_ptr(), cl.data_ptr(), 0.0, None, 1.0, o[0], o[0],
                                   o[0], P, 1 << 18, st) == -2
        torch.cuda.synchronize()
        assert bool((out == 7.25).all()) and bool((ws == 0x5A).all())
    assert eng.multilabel_f32_supported(eng.Tables("distmult", ent, rel))


def _random_csr(n, E, gen, mean=8):
    k = torch.randint(0, 2 * mean + 1, (n,), generator=gen)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(k, 0)
    col = torch.cat([torch.randperm(E, generator=gen)[:int(x)] for x in k])
    return rowptr.to(DEV), col.to(DEV)


def _model_loss(m, kind, direction, q, p, rowptr, col, eps):
    if kind == "kl":
        return m.kl_loss_sp(q, p, rowptr, col, eps) if direction == "sp" else m.kl_loss_po(p, q, rowptr, col, eps)
    return (m.bce_loss_sp(q, p, rowptr, col, 2.0, eps) if direction == "sp"
            else m.bce_loss_po(p, q, rowptr, col, 2.0, eps))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["kl", "bce"])
@pytest.mark.parametrize("name", ["complex", "distmult"])
def test_model_level_one_sgd_step_fused_against_composed(monkeypatch, name, kind, eps):
    """km.create(..., fused_f32_loss=True) against fused_f32_loss=False from identical parameters, both directions: the
    loss and the parameters after one SGD step, each within 4 x the composed model's own error against the float64 step
    (KgeModel._kl_composed / _bce_composed on float64 scores)."""
    from kge_amd import model as km
    E, R, d, n, lr = 3005, 11, 64, 300, 0.5
    gen = torch.Generator().manual_seed(2)
    q, p = (torch.randint(hi, (n,), generator=gen).to(DEV) for hi in (E, R))
    rowptr, col = _random_csr(n, E, gen)
    entered = []
    for cls in (km._FusedKLF32, km._FusedBCEF32):
        def forward(ctx, *a, _orig=cls.forward, _name=cls.__name__):
            entered.append(_name)
            return _orig(ctx, *a)
        monkeypatch.setattr(cls, "forward", staticmethod(forward))
    for direction in DIRECTIONS:
        res = {}
        for fused in (True, False):
            torch.manual_seed(0)
            m = km.create(name, E, R, d, device=DEV, fused_f32_loss=fused).train()
            assert (m._ce_f32_tables() is not None) == fused
            we, wr = m.get_s_embedder().weight, m.get_p_embedder().weight
            if fused:
                e64, r64 = we.detach().double().cpu().requires_grad_(), wr.detach().double().cpu().requires_grad_()
            opt = torch.optim.SGD(m.parameters(), lr=lr)
            before = len(entered)
            total = _model_loss(m, kind, direction, q, p, rowptr, col, eps).sum() / n
            assert len(entered) - before == int(fused), entered
            total.backward()
            opt.step()
            res[fused] = (float(total), we.detach().double().cpu(), wr.detach().double().cpu())
        qc, pc = q.cpu(), p.cpu()
        sc = tp.score_sp(name, e64, r64, qc, pc) if direction == "sp" else tp.score_po(name, e64, r64, pc, qc)
        rows = (km.KgeModel._kl_composed(sc, rowptr.cpu(), col.cpu(), eps) if kind == "kl"
                else km.KgeModel._bce_composed(sc, rowptr.cpu(), col.cpu(), 2.0, eps))
        t64 = rows.sum() / n
        t64.backward()
        want = (float(t64), (e64 - lr * e64.grad).detach(), (r64 - lr * r64.grad).detach())
        (lf, ef, rf), (lc, ec, rc) = res[True], res[False]
        for nm, f, cm, w in (("loss", lf, lc, want[0]), ("entity", ef, ec, want[1]), ("relation", rf, rc, want[2])):
            errf, errc = (abs(f - w), abs(cm - w)) if nm == "loss" else (float((f - w).abs().max()), float((cm - w).abs().max()))
            print(f"MODEL {name} {kind} eps {eps} {direction} {nm}: vs float64 fused {errf:.3e} composed {errc:.3e}")
            assert errf <= 4 * max(errc, EPS * max(1.0, abs(w) if nm == "loss" else float(w.abs().max()))), (nm, errf, errc)
    assert entered == ["_FusedKLF32" if kind == "kl" else "_FusedBCEF32"] * 2, entered


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["kl", "bce"])
def test_memory_bound_of_a_model_step(kind, eps):
    """n = 256, E = 131,072, d = 16: one [n, E] float32 matrix is 4 n E = 128 MB; the composed path holds at least three
    (scores, labels, the loss's intermediate; then their gradients).  The fused step raises max_memory_allocated by less
    than ONE over what is held after a warm-up step (the cached workspace, .grad)."""
    from kge_amd import model as km
    E, R, d, n = 131072, 7, 16, 256
    torch.manual_seed(0)
    m = km.create("complex", E, R, d, device=DEV, fused_f32_loss=True).train()
    assert m._ce_f32_tables() is not None
    gen = torch.Generator().manual_seed(1)
    s, p = (torch.randint(hi, (n,), generator=gen).to(DEV) for hi in (E, R))
    rowptr, col = _random_csr(n, E, gen)
    step = lambda: _model_loss(m, kind, "sp", s, p, rowptr, col, eps)
    step().sum().backward()  # warm-up: workspace and .grad exist from here on
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=False)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rows = step()
    rows.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"MEM fused {kind} eps {eps} step: peak rise {rise / 2**20:.1f} MB over {base / 2**20:.1f} MB held "
          f"(one [n, E] float32 matrix: {4 * n * E / 2**20:.0f} MB)")
    assert bool(torch.isfinite(rows).all()) and rise < 4 * n * E, rise
