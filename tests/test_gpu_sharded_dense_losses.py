"""The dense-row loss kernels of entity-sharded training on the GPU, shard by shard, against float64:
kge_ce_emb_fwd / _bwd, kge_kl_weighted_emb_fwd / _bwd, kge_bce_emb_fwd / _bwd (engine.ce_emb_*, kl_emb_*, bce_emb_*).

One process, one GPU, no collectives: the whole bf16 table lives on the device, every shard [lo, hi) of an explicit cut
list is engine.Tables(model, ent16[lo:hi], rel16) with col_lo = lo, and every shard runs the real kernels -- so the
in-range test of the label kernels at col_lo != 0, rows whose labels all belong to another shard, the count of labels in
range (bce), a backward fed a GLOBAL log-sum-exp, label_bias (label smoothing) and query rows with a row stride above
dim are all on the device.  The cut lists give the scoring kernels shard sizes of 3, 65, 64 and 905 (a tiny shard,
m % 64 == 1, exactly one tile, a ragged multi-tile one) and 1027 / 973; the row counts reach the single-role kernel
(d = 128), the loader/consumer kernel (37 and 300 rows at d in {256, 512}; 300 = three row groups) and the persistent
kernel (160 rows).

References (tests/_sharded_dense_ref.py, checked on the CPU by tests/test_sharded_dense_ref_cpu.py):
  * forward, "tables": float64 scores of the bf16-valued tables with the query rounded to bf16 the way the project's
    bf16 semantics define a score (oracle/kge_oracle.c; the kernels hold q as a bf16 matrix operand) -- independent of
    every GPU kernel; what differs from the kernels is float32 accumulation, exp / log and summation order;
  * forward, "written": float64 of the scores engine.score_sp / score_po write for the whole table (the same score bits
    as inside the fused kernels);
  * backward: float64 autograd over the whole table (query NOT rounded: the mixed-precision bar of test_gpu_ce.py).
Forward bounds (test_gpu_ce.py's for the same kernels; want = the float64 value, amax = the row's largest |score| in the
shard, k = the row's labels in the shard):
    lse                  1e-5 + 1e-5 |want|
    kl loss rows         1e-5 + 1e-5 |lse| + |w_i| 2e-6 amax k
    bce loss rows        1e-5 |want| + 1e-4 + 2e-6 amax k
    ce loss rows (own)   the lse bound + 2e-6 amax
and for the merged global loss (lse merged, terms summed, in float64) the shards' bounds summed.  Backward: relative
Frobenius error <= 1e-2 of the concatenated shard gradients and of the summed query-row gradients (measured: at most
2.9e-3), and the per-row relative error PER_ROW_TOL = 3.86e-2 = 4 x the largest measured on an MI355X, 9.65e-3 (see
PER_ROW_MEASURED below), on the entity rows next to every cut (and rows 0, E - 1), and on the query rows of the 70-label
row and of the rows whose labels all lie in one shard: every border entity is a label of at most three rows, so a
dropped label moves its gradient row by a large part of its norm (a float64 backward that skips the first row of
every shard at lo > 0 is 9 % to 35 % off on that row in every case below, several times the cap on PER_ROW_TOL, 5e-2) --
which a whole-table norm can hide.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _sharded_dense_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# The largest per-row relative error of a gradient row against float64 autograd, measured on an MI355X over every case
# below (all three losses, smoothing, the whole-table kl_bwd): 9.65e-3, an entity row of the bce loss in the ONE-row case
# -- the row is a single product G_0j q_0 of two bf16-rounded factors, and on a label column G = bf16(bf16(g sigmoid) - g)
# keeps the absolute rounding error of g sigmoid on the smaller g (sigmoid - 1): 2^-9 sigmoid / (1 - sigmoid) relative.
# With more rows: 5.4e-3 (ce), 4.0e-3 (kl), 3.4e-3 (bce, smoothed kl).  The bound is four times the largest (the margin
# is for another summation order in the products); the issue's cap on it is 5e-2.
PER_ROW_MEASURED = 9.65e-3
PER_ROW_TOL = 4 * PER_ROW_MEASURED

LAYOUTS = {"A": (1037, [0, 3, 68, 132, 1037]), "B": (2000, [0, 1027, 2000])}
R = 7
CASES = [  # model, d, n, cut layout, scale (scores of order 1)          kernel of the loss passes
    ("complex", 512, 37, "A", 0.3),      # loader/consumer
    ("distmult", 256, 300, "A", 0.5),    # loader/consumer, three row groups
    ("complex", 256, 160, "A", 0.3),     # persistent
    ("distmult", 512, 160, "B", 0.3),    # persistent
    ("complex", 128, 37, "B", 0.5),      # single-role
    ("distmult", 128, 1, "A", 0.5),      # single-role, one row
    ("complex", 512, 300, "B", 0.3),     # loader/consumer, three row groups
    ("distmult", 256, 37, "B", 0.5),     # loader/consumer
]
SCALAR_CASE = CASES[0]  # the backward called with g_rows = None and a g_scalar
_ids = lambda c: f"{c[0]}-d{c[1]}-n{c[2]}-{c[3]}"
case_param = pytest.mark.parametrize("case", CASES, ids=_ids)


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _report(name, value):
    print(f"MEASURED {name} {value:.3e}")


def _dev(x, dtype=None):
    t = torch.as_tensor(x)
    return (t if dtype is None else t.to(dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _setup(case):
    """Everything of a case that does not depend on the loss: tables, shards, query rows (contiguous and strided),
    labels, upstream gradients and both forward references per direction -- built once, read by every test."""
    from kge_amd import engine as eng
    model, d, n, layout, scale = case
    E, cuts = LAYOUTS[layout]
    seed = 1000 * d + 10 * n + E
    g = torch.Generator().manual_seed(seed)
    ent = (torch.randn(E, d, generator=g) * scale).bfloat16()
    rel = (torch.randn(R, d, generator=g) * scale).bfloat16()
    a, p = torch.randint(E, (n,), generator=g), torch.randint(R, (n,), generator=g)
    rng = np.random.default_rng(seed)
    bnd = ref.boundary_ids(cuts)
    if n >= ref.MIN_ROWS:
        rowptr, col, info = ref.make_labels(rng, n, E, cuts)
        qrows = [info["many"], info["one_shard"], info["elsewhere"]]
        none_row = info["none"]
        lab = rng.integers(0, E, n)
        lab[np.round(np.linspace(0, n - 1, len(bnd))).astype(int)] = bnd   # 1vsAll labels on both sides of every cut
    else:  # one row: a boundary row (labels on both sides of every cut, so in every shard)
        rp, cl, info = ref.make_labels(rng, ref.MIN_ROWS, E, cuts)
        rowptr, col = ref.take_rows(rp, cl, [info["boundary"][1]] * n)
        qrows, none_row, info = [0], None, None
        lab = np.full(n, cuts[1])
    c = SimpleNamespace(model=model, d=d, n=n, E=E, cuts=cuts, shards=list(zip(cuts, cuts[1:])), bnd=bnd, info=info,
                        qrows=qrows, none_row=none_row, rowptr=rowptr, col=col, lab=torch.from_numpy(lab),
                        ent=ent, rel=rel, a=a, p=p)
    c.ent_d, c.rel_d, c.a_d, c.p_d = ent.to(DEV), rel.to(DEV), a.to(DEV), p.to(DEV)
    c.rowptr_d, c.col_d = _dev(rowptr), _dev(col)
    c.T = eng.Tables(model, c.ent_d, c.rel_d)
    c.Ts = [eng.Tables(model, c.ent_d[lo:hi], c.rel_d) for lo, hi in c.shards]
    assert all(eng.ce_supported(t) for t in c.Ts)
    c.g = (torch.rand(n, generator=g) + 0.5) / n          # float32, [0.5, 1.5) / n
    c.a_rows, c.p_rows = ent[a], rel[p]                    # bf16, CPU
    c.a_rows_d, c.p_rows_d = c.a_rows.to(DEV), c.p_rows.to(DEV)

    def strided(rows):  # the same rows out of a wider buffer: row stride d + 8, base 8 elements (16 bytes) in
        buf = torch.full((n * (d + 8) + 8,), float("nan"), dtype=torch.bfloat16, device=DEV)
        v = buf[8:].view(n, d + 8)[:, :d]
        v.copy_(rows)
        assert v.stride(0) == d + 8 and v.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + 16
        return v

    c.a_strided, c.p_strided = strided(c.a_rows_d), strided(c.p_rows_d)
    c.x = {}
    for direction in ("sp", "po"):
        written = eng.score_sp(c.T, c.a_d, c.p_d) if direction == "sp" else eng.score_po(c.T, c.p_d, c.a_d)
        c.x[direction] = {"tables": ref.scores64(model, direction, c.a_rows, c.p_rows, ent, q_bf16=True),
                          "written": written.cpu().double()}
    return c


def _check(name, got, want, tol):
    err = (got.double().cpu() - want).abs()
    if err.numel() == 0:
        return
    _report(name + " err/bound", float((err / tol).max()))
    assert bool((err <= tol).all()), (name, float(err.max()), int((err > tol).sum()))


def _lse_tol(want):
    return 1e-5 + 1e-5 * want.abs()


def _check_grads(tag, c, got, want, qrows):
    """got = (g_a, g_p: the shards' summed; g_t: the shards' concatenated), want = float64 autograd's."""
    for nm, x, w in zip(("g_a", "g_p", "g_t"), got, want):
        x = x.double().cpu()
        assert x.shape == w.shape and bool(torch.isfinite(x).all()), (tag, nm)
        rel_err = float((x - w).norm() / w.norm())
        _report(f"{tag} {nm} frobenius", rel_err)
        assert rel_err <= 1e-2, (tag, nm, rel_err)
    for nm, x, w, rows in (("g_t", got[2], want[2], c.bnd), ("g_a", got[0], want[0], qrows)):
        x, w = x.double().cpu()[rows], w[rows]
        err = (x - w).norm(dim=1) / w.norm(dim=1)
        _report(f"{tag} {nm} per-row", float(err.max()))
        assert bool((err <= PER_ROW_TOL).all()), (tag, nm, [int(r) for r in rows], err.tolist())


def _sum64(xs):
    return sum(x.double() for x in xs)


def _g(c, scalar, g=None):
    """(g_rows on the device or None, g_scalar, the float64 row gradients the reference takes); scalar: the upstream
    gradient as g_rows = None and a g_scalar."""
    if scalar:
        gs = float(np.float32(1.0 / c.n))
        return None, gs, torch.full((c.n,), gs, dtype=torch.float64)
    g = c.g if g is None else g
    return g.to(DEV), 1.0, g.double()


# ---- 1vsAll ------------------------------------------------------------------------------------------------------------
@case_param
def test_ce_shards(eng, case):
    """kge_ce_emb_fwd / _bwd per shard.  The loss row is NaN exactly where another shard owns the label (passed as -1 and
    as m), the lse finite there; per-shard and merged values within the bounds of the module docstring, against both
    references and against the unsharded kge_ce_fwd; the backward, fed the merged global lse, against float64 autograd."""
    c = _setup(case)
    odd = torch.arange(c.n) % 2 == 1
    for direction in ("sp", "po"):
        parts, locs, tol_sum = [], [], 0.0
        for (lo, hi), T in zip(c.shards, c.Ts):
            m = hi - lo
            own = (c.lab >= lo) & (c.lab < hi)
            loc = torch.where(own, c.lab - lo, torch.where(odd, torch.full_like(c.lab, -1), torch.full_like(c.lab, m)))
            loss, lse = eng.ce_emb_fwd(T, direction, c.a_rows_d, c.p_rows_d, loc.to(DEV))
            loss, lse = loss.cpu(), lse.cpu()
            assert torch.equal(torch.isnan(loss), ~own) and bool(torch.isfinite(lse).all()), (direction, lo)
            for tag, x in c.x[direction].items():
                xs = x[:, lo:hi]
                want_loss, want_lse = ref.ce64(xs, loc)
                tol = _lse_tol(want_lse)
                _check(f"ce {direction} [{lo},{hi}) {tag} lse", lse, want_lse, tol)
                tol_own = tol + 2e-6 * xs.abs().max(1).values
                _check(f"ce {direction} [{lo},{hi}) {tag} loss", loss[own], want_loss[own], tol_own[own])
                if tag == "tables":
                    tol_sum = tol_sum + torch.where(own, tol_own, tol)
            parts.append((loss, lse))
            locs.append(loc.to(DEV))
        loss, lse = ref.merge_ce(*zip(*parts))
        x = c.x[direction]["tables"]
        want_lse = torch.logsumexp(x, 1)
        _check(f"ce {direction} merged lse", lse, want_lse, tol_sum)
        _check(f"ce {direction} merged loss", loss, want_lse - x.gather(1, c.lab.view(-1, 1)).view(-1), tol_sum)
        u_loss, u_lse = eng.ce_fwd(c.T, direction, c.a_d, c.p_d, c.lab.to(DEV))
        _check(f"ce {direction} merged lse / unsharded", lse, u_lse.double().cpu(), tol_sum)
        _check(f"ce {direction} merged loss / unsharded", loss, u_loss.double().cpu(), tol_sum)
        # backward with the global lse
        lse_d = lse.float().to(DEV)
        g_d, gs, g64 = _g(c, case == SCALAR_CASE)
        outs = [eng.ce_emb_bwd(T, direction, c.a_rows_d, c.p_rows_d, loc, lse_d, g_rows=g_d, g_scalar=gs)
                for T, loc in zip(c.Ts, locs)]
        got = (_sum64([o[0] for o in outs]), _sum64([o[1] for o in outs]), torch.cat([o[2] for o in outs]))
        want = ref.ce_grads64(c.model, direction, c.a_rows, c.p_rows, c.ent, c.lab, g64)
        _check_grads(f"ce {direction}", c, got, want, sorted({0, c.n - 1}))


# ---- KvsAll, kl --------------------------------------------------------------------------------------------------------
def _run_kl(eng, c, case, direction, w, bias, has):
    """Forward per shard and merged; backward per shard with the merged lse.  -> (lse_d, g_d, gs, want)"""
    w_d = w.to(DEV)
    parts, tol_sum = [], 0.0
    for (lo, hi), T in zip(c.shards, c.Ts):
        loss, lse = eng.kl_emb_fwd(T, direction, c.a_rows_d, c.p_rows_d, c.rowptr_d, c.col_d, lo, w_d)
        loss, lse = loss.cpu(), lse.cpu()
        for tag, x in c.x[direction].items():
            xs = x[:, lo:hi]
            want_loss, want_lse, k = ref.kl_weighted64(xs, c.rowptr, c.col, lo, w)
            _check(f"kl {direction} [{lo},{hi}) {tag} lse", lse, want_lse, _lse_tol(want_lse))
            tol = 1e-5 + 1e-5 * want_lse.abs() + w.double().abs() * 2e-6 * xs.abs().max(1).values * k
            _check(f"kl {direction} [{lo},{hi}) {tag} loss", loss, want_loss, tol)
            if tag == "tables":
                tol_sum = tol_sum + tol
        assert torch.equal(loss[k == 0], lse[k == 0]), (direction, lo)   # no label in this shard: the lse itself
        if c.info is not None:   # (the edge is there: a row with labels, all of them another shard's)
            assert bool(((k == 0) & torch.from_numpy(np.diff(c.rowptr) > 0)).any()), (direction, lo)
        parts.append((loss, lse))
    loss, lse = ref.merge_kl(*zip(*parts))
    want_loss, want_lse, k = ref.kl_weighted64(c.x[direction]["tables"], c.rowptr, c.col, 0, w)
    assert torch.equal(k, torch.from_numpy(np.diff(c.rowptr)).double())
    _check(f"kl {direction} merged lse", lse, want_lse, tol_sum)
    _check(f"kl {direction} merged loss", loss, want_loss, tol_sum)
    u_loss, u_lse = eng.kl_fwd(c.T, direction, c.a_d, c.p_d, c.rowptr_d, c.col_d, label_weight=w_d)
    _check(f"kl {direction} merged loss / unsharded", loss, u_loss.double().cpu(), tol_sum)
    lse_d = lse.float().to(DEV)
    # as _ShardedKL.backward: rows without labels get no gradient -- unless the labels are smoothed
    # (a scalar cannot zero single rows: only where every row has label mass)
    g_d, gs, g64 = _g(c, case == SCALAR_CASE and bool(has.all()), torch.where(has, c.g, torch.zeros_like(c.g)))
    bias_d = None if bias is None else bias.to(DEV)
    outs = [eng.kl_emb_bwd(T, direction, c.a_rows_d, c.p_rows_d, c.rowptr_d, c.col_d, lo, w_d, lse_d, g_rows=g_d,
                           g_scalar=gs, label_bias=bias_d) for (lo, hi), T in zip(c.shards, c.Ts)]
    got = (_sum64([o[0] for o in outs]), _sum64([o[1] for o in outs]), torch.cat([o[2] for o in outs]))
    want = ref.kl_grads64(c.model, direction, c.a_rows, c.p_rows, c.ent, c.rowptr, c.col, w, g64, bias)
    _check_grads(f"kl {direction}" + ("" if bias is None else " smoothed"), c, got, want, c.qrows)
    return outs, got, want, (u_lse, g_d, gs, w_d, bias_d)


@case_param
def test_kl_shards(eng, case):
    """kge_kl_weighted_emb_fwd / _bwd per shard without smoothing (w = 1 / k): a row with no label in a shard has
    loss == lse there, bit for bit; a row without labels gets an exactly zero g_a / g_p row from every shard when the
    caller zeroes its g (its reference gradient is zero as well)."""
    from kge_amd import sharded
    c = _setup(case)
    _k, has, w, bias, _const = sharded._kl_label_terms(torch.from_numpy(c.rowptr), 0.0, c.E)
    assert bias is None
    for direction in ("sp", "po"):
        outs, got, want, _ = _run_kl(eng, c, case, direction, w, None, has)
        if c.none_row is not None:
            for g_a, g_p, _g_t in outs:
                assert float(g_a[c.none_row].abs().max()) == 0.0 and float(g_p[c.none_row].abs().max()) == 0.0
            assert float(want[0][c.none_row].abs().max()) == 0.0


@case_param
def test_kl_shards_with_label_smoothing(eng, case):
    """label_bias in kge_kl_weighted_emb_bwd (w, bias of sharded._kl_label_terms, eps = 0.1): the uniform mass is
    subtracted at every column of every shard, rows without labels get a gradient; and the same reference for the
    whole-table kge_kl_weighted_bwd (engine.kl_bwd(label_weight=, label_bias=))."""
    from kge_amd import sharded
    c = _setup(case)
    _k, has, w, bias, _const = sharded._kl_label_terms(torch.from_numpy(c.rowptr), 0.1, c.E)
    assert bias is not None and bool(has.all())
    for direction in ("sp", "po"):
        outs, got, want, (u_lse, g_d, gs, w_d, bias_d) = _run_kl(eng, c, case, direction, w, bias, has)
        if c.none_row is not None:
            assert float(got[0][c.none_row].norm()) > 0.0 and float(want[0][c.none_row].norm()) > 0.0
        u = eng.kl_bwd(c.T, direction, c.a_d, c.p_d, c.rowptr_d, c.col_d, u_lse, g_rows=g_d, g_scalar=gs,
                       label_weight=w_d, label_bias=bias_d)
        _check_grads(f"kl {direction} smoothed, whole table", c, u, want, c.qrows)


# ---- KvsAll, bce -------------------------------------------------------------------------------------------------------
@case_param
def test_bce_shards(eng, case):
    """kge_bce_emb_fwd / _bwd per shard (the only user of kl_label_kernel's count of labels in range: the offset enters
    once per label IN the shard): a row with no label in a shard gives the bits of the same row under an empty CSR."""
    c = _setup(case)
    offset = (-0.5, 0.0)[c.n % 2]
    empty_rp, empty_cl = torch.zeros(c.n + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)
    for direction in ("sp", "po"):
        parts, tol_sum = [], 0.0
        for (lo, hi), T in zip(c.shards, c.Ts):
            loss = eng.bce_emb_fwd(T, direction, c.a_rows_d, c.p_rows_d, c.rowptr_d, c.col_d, lo, offset).cpu()
            for tag, x in c.x[direction].items():
                xs = x[:, lo:hi]
                want, k = ref.bce64(xs, c.rowptr, c.col, lo, offset)
                tol = 1e-5 * want.abs() + 1e-4 + 2e-6 * xs.abs().max(1).values * k
                _check(f"bce {direction} [{lo},{hi}) {tag} loss", loss, want, tol)
                if tag == "tables":
                    tol_sum = tol_sum + tol
            bare = eng.bce_emb_fwd(T, direction, c.a_rows_d, c.p_rows_d, empty_rp, empty_cl, lo, offset).cpu()
            assert torch.equal(loss[k == 0], bare[k == 0]), (direction, lo)
            assert c.info is None or not torch.equal(loss, bare)
            parts.append(loss)
        loss = ref.merge_bce(parts)
        want, k = ref.bce64(c.x[direction]["tables"], c.rowptr, c.col, 0, offset)
        _check(f"bce {direction} merged loss", loss, want, tol_sum)
        u = eng.bce_fwd(c.T, direction, c.a_d, c.p_d, c.rowptr_d, c.col_d, offset)
        _check(f"bce {direction} merged loss / unsharded", loss, u.double().cpu(), tol_sum)
        g_d, gs, g64 = _g(c, case == SCALAR_CASE)
        outs = [eng.bce_emb_bwd(T, direction, c.a_rows_d, c.p_rows_d, c.rowptr_d, c.col_d, lo, offset, g_rows=g_d,
                                g_scalar=gs) for (lo, hi), T in zip(c.shards, c.Ts)]
        got = (_sum64([o[0] for o in outs]), _sum64([o[1] for o in outs]), torch.cat([o[2] for o in outs]))
        want = ref.bce_grads64(c.model, direction, c.a_rows, c.p_rows, c.ent, c.rowptr, c.col, offset, g64)
        _check_grads(f"bce {direction}", c, got, want, c.qrows)


# ---- bit-for-bit properties ----------------------------------------------------------------------------------------------
def _all_losses(eng, c, T, lo, direction, a_rows, p_rows, rowptr_d, col_d, w_d, bias_d, lse_d, loc_d, g_d):
    """Every output of the six entry points on one shard, as a flat list."""
    out = []
    out += eng.ce_emb_fwd(T, direction, a_rows, p_rows, loc_d)
    out += eng.ce_emb_bwd(T, direction, a_rows, p_rows, loc_d, lse_d, g_rows=g_d)
    out += eng.kl_emb_fwd(T, direction, a_rows, p_rows, rowptr_d, col_d, lo, w_d)
    out += eng.kl_emb_bwd(T, direction, a_rows, p_rows, rowptr_d, col_d, lo, w_d, lse_d, g_rows=g_d, label_bias=bias_d)
    out += [eng.bce_emb_fwd(T, direction, a_rows, p_rows, rowptr_d, col_d, lo, -0.5)]
    out += eng.bce_emb_bwd(T, direction, a_rows, p_rows, rowptr_d, col_d, lo, -0.5, g_rows=g_d)
    return out


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _bitwise_inputs(c):
    from kge_amd import sharded
    _k, _has, w, bias, _const = sharded._kl_label_terms(torch.from_numpy(c.rowptr), 0.1, c.E)
    lse_d = torch.logsumexp(c.x["sp"]["written"], 1).float().to(DEV)   # some global lse: the same in both runs
    return w.to(DEV), bias.to(DEV), lse_d, c.g.to(DEV)


@case_param
def test_strided_query_rows_give_the_same_bits(eng, case):
    """a_ld = p_ld = dim + 8 and a base 16 bytes into its buffer (what ce_supported asks for: a 16-byte aligned base,
    ld % 8 == 0) against contiguous rows: all six entry points, every shard, bit for bit."""
    c = _setup(case)
    w_d, bias_d, lse_d, g_d = _bitwise_inputs(c)
    for direction in ("sp", "po"):
        for (lo, hi), T in zip(c.shards, c.Ts):
            loc_d = torch.where((c.lab >= lo) & (c.lab < hi), c.lab - lo, torch.full_like(c.lab, -1)).to(DEV)
            args = (c.rowptr_d, c.col_d, w_d, bias_d, lse_d, loc_d, g_d)
            plain = _all_losses(eng, c, T, lo, direction, c.a_rows_d, c.p_rows_d, *args)
            wide = _all_losses(eng, c, T, lo, direction, c.a_strided, c.p_strided, *args)
            for k, (x, y) in enumerate(zip(plain, wide)):
                assert _same_bits(x, y), (direction, lo, k)


@case_param
def test_label_ids_no_shard_owns_change_nothing(eng, case):
    """Negative control: ids >= E and < 0 in the CSR (also as the ONLY entries of the row without labels, and one that
    is 0 modulo 2^32) are skipped by every shard: losses and gradients bit for bit those of the CSR without them."""
    c = _setup(case)
    w_d, bias_d, lse_d, g_d = _bitwise_inputs(c)
    if c.info is not None:
        extra = {c.info["none"]: [c.E, -3], c.info["many"]: [c.E + 5], c.info["boundary"][0]: [-1, 1 << 40],
                 c.info["k4"]: [-(1 << 33)], c.n - 1: [c.E]}
    else:
        extra = {0: [c.E, -1, 1 << 40]}
    rp2, cl2 = ref.with_extra_labels(c.rowptr, c.col, extra)
    assert len(cl2) == len(c.col) + sum(len(v) for v in extra.values())
    rp2_d, cl2_d = _dev(rp2), _dev(cl2)
    for direction in ("sp", "po"):
        for (lo, hi), T in zip(c.shards, c.Ts):
            loc_d = torch.full((c.n,), -1, dtype=torch.int64, device=DEV)
            rest = (w_d, bias_d, lse_d, loc_d, g_d)
            clean = _all_losses(eng, c, T, lo, direction, c.a_rows_d, c.p_rows_d, c.rowptr_d, c.col_d, *rest)
            dirty = _all_losses(eng, c, T, lo, direction, c.a_rows_d, c.p_rows_d, rp2_d, cl2_d, *rest)
            for k, (x, y) in enumerate(zip(clean, dirty)):
                assert _same_bits(x, y), (direction, lo, k)
