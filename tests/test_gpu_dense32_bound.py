"""The fused float32 losses of TransE / RotatE (kge_ce_dist_*, kge_kl_dist_*, kge_bce_dist_*: ce_dist.hip) and of float32
ComplEx / DistMult tables (kge_ce_f32_*, kge_kl_f32_*, kge_bce_f32_*: ce_f32.hip, score_pairs_f32.hip) on the MI355X,
held elementwise to the float64 restatement of tests/_dense32_ref.py with its counted bounds, on the planted rows of
CASES_DIST and CASES_F32 -- the walked shapes WALK_DIST (col_tiles = 3) and WALK_F32 (col_tiles = 2), each with a short
last group, among them, asserted from the library's own workspace sizes.  tests/test_dense32_ref_cpu.py checks the same
inputs, the bounds and the planted defects without a GPU.

Per case and direction: the stored score bits equal the oracle's; lse and loss_rows lie inside the forward bound of float64
on those bits; two runs give identical forward outputs; g_a, g_p, g_tgt lie elementwise inside the gradient bound at the
smallest chunk width (64 / 128) and at the default; g_tgt is bit-equal between the two; kl_f32_fwd's lse is bit-equal to
ce_f32_fwd's.  The backward is given the float32 rounding of the float64 lse, as the reference is."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _dense32_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ALL = [(c, d) for c in D.CASES for d in D.directions(c)]
IDS = [f"{D.case_id(c)}-{d}" for c, d in ALL]


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(idx, direction):
    """inputs and the float64 references of one case, computed once and shared (never modified)"""
    k = D.make_case(D.CASES[idx], direction)
    x32 = D.oracle_scores(k)
    lse32 = D.ref_lse32(x32)
    P, e = D.coef64(k, x32, lse32), D.coef_radius(k, x32, lse32)
    want, bound = D.grads_and_bound(k, P, e)
    loss, z = D.loss64(k, x32)
    return dict(k=k, x32=x32, lse32=lse32, want=want, bound=bound, loss=loss, z=z, b_loss=D.loss_bound(k, x32),
                b_lse=D.lse_bound(x32, k["n"], k["name"]))


def _fam(k):
    return "f32" if k["name"] in D.F32 else "dist"


def _fwd(eng, T, k):
    ai, pi, dr = _t(k["a"]), _t(k["p"]), k["direction"]
    fn = lambda what: getattr(eng, f"{what}_{_fam(k)}_fwd")
    if k["kind"] == "ce":
        return fn("ce")(T, dr, ai, pi, _t(k["label"]))
    if k["kind"] == "kl":
        lw = None if k.get("label_weight") is None else _t(k["label_weight"])
        return fn("kl")(T, dr, ai, pi, _t(k["rowptr"]), _t(k["col"]), lw)
    return fn("bce")(T, dr, ai, pi, _t(k["rowptr"]), _t(k["col"]), k["offset"]), None


def _bwd(eng, T, k, lse, chunk_cols):
    ai, pi, dr = _t(k["a"]), _t(k["p"]), k["direction"]
    g = {"g_scalar": k["g_scalar"]} if k.get("g_rows") is None else {"g_rows": _t(k["g_rows"])}
    fn = lambda what: getattr(eng, f"{what}_{_fam(k)}_bwd")
    if k["kind"] == "ce":
        return fn("ce")(T, dr, ai, pi, _t(k["label"]), lse, chunk_cols=chunk_cols, **g)
    if k["kind"] == "kl":
        lw = None if k.get("label_weight") is None else _t(k["label_weight"])
        if k.get("label_bias") is not None:
            g["label_bias"] = _t(k["label_bias"])
        return fn("kl")(T, dr, ai, pi, _t(k["rowptr"]), _t(k["col"]), lse, label_weight=lw, chunk_cols=chunk_cols, **g)
    return fn("bce")(T, dr, ai, pi, _t(k["rowptr"]), _t(k["col"]), k["offset"], chunk_cols=chunk_cols, **g)


def _inside(tag, got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(err == 0, 0.0, err / bound)))
    print(f"dense32 {tag}: max err / bound {ratio:.3g} (max err {float(err.max()):.3g})")
    assert np.isfinite(np.asarray(got)).all(), tag
    assert (err <= bound).all(), (tag, ratio, int((err > bound).sum()))


def _tables(eng, k):
    ent = _t(k["ent"])
    if k.get("ent_ld", 0) > ent.shape[1]:  # rows on a wider pitch: a view into an [E, ent_ld] buffer of NaN
        buf = torch.full((ent.shape[0], k["ent_ld"]), float("nan"), device=DEV)
        buf[:, :ent.shape[1]] = ent
        ent = buf[:, :k["ent"].shape[1]]
    return eng.Tables(k["name"], ent, _t(k["rel"]), k["l_norm"])


def test_walk_dist_takes_three_column_tiles_and_a_short_last_group(eng):
    """From kge_ce_dist_workspace_bytes: the record block of WALK_DIST is 12 n G bytes with G = 172 (171 and 173 give other
    sizes); 514 tiles in 172 groups is col_tiles = 3 (2 would give 257 groups, 4 would give 129), and 171 * 3 tiles end one
    column before E: the last group is one tile with one valid column."""
    from kge_amd import _lib
    d, E, n = D.WALK_DIST
    T = eng.Tables("transe", torch.zeros(E, d, device=DEV), torch.zeros(3, d, device=DEV), 1.0)
    al = lambda b: -(-b // 256) * 256
    rec = _lib.lib().kge_ce_dist_workspace_bytes(ctypes.byref(T.c()), n, 64) - al(4 * n * d) - al(4 * n * 64)
    assert rec == al(12 * n * 172) and rec not in (al(12 * n * 171), al(12 * n * 173))
    assert rec == D.records_bytes(n, E) and D.cd_groups(n, E) == (3, 172)
    assert -(-514 // 3) == 172 and -(-514 // 2) == 257 and -(-514 // 4) == 129 and 171 * 3 * 64 == E - 1


def test_walk_f32_takes_two_column_tiles_and_a_short_last_group(eng):
    """From kge_ce_f32_workspace_bytes (the layout of tests/test_gpu_ce_f32.py): 151 record groups per row; 301 tiles in
    151 groups is col_tiles = 2, and 150 * 2 tiles end one column before E."""
    from kge_amd import _lib
    d, E, n, _ = D.WALK_F32
    T = eng.Tables("complex", torch.zeros(E, d, device=DEV), torch.zeros(3, d, device=DEV))
    al = lambda b: -(-b // 256) * 256
    fixed = _lib.lib().kge_ce_f32_workspace_bytes(ctypes.byref(T.c()), n, 128) - 4 * n * 128
    assert fixed == al(12 * n * 151) + 2 * al(4 * n * d) + al(32 * 4 * n * d), fixed
    assert al(12 * n * 151) not in (al(12 * n * 150), al(12 * n * 152)) and D.cf_groups(n, E) == (2, 151)
    assert -(-301 // 2) == 151 and -(-301 // 3) == 101 and 150 * 2 * 128 == E - 1


@pytest.mark.parametrize("idx,direction", [(D.CASES.index(c), d) for c, d in ALL], ids=IDS)
def test_forward_and_backward_inside_the_float64_bounds(eng, idx, direction):
    r = _ref(idx, direction)
    k = r["k"]
    tag = f"{D.case_id(D.CASES[idx])} {direction}"
    T = _tables(eng, k)
    ai, pi = _t(k["a"]), _t(k["p"])
    sc = (eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)).cpu().numpy()
    assert np.array_equal(sc, r["x32"]), "stored scores differ from the oracle's bits"
    loss, lse = _fwd(eng, T, k)
    loss2, lse2 = _fwd(eng, T, k)
    assert torch.equal(loss, loss2) and (lse is None or torch.equal(lse, lse2)), "two runs differ"
    if lse is not None:
        _inside(f"{tag} lse", lse.cpu().numpy(), r["z"], r["b_lse"])
    if k["kind"] == "kl" and _fam(k) == "f32":
        _, lse_ce = eng.ce_f32_fwd(T, direction, ai, pi, torch.zeros_like(ai))
        assert torch.equal(lse, lse_ce), "kl_f32_fwd's lse differs from ce_f32_fwd's"
    _inside(f"{tag} loss_rows", loss.cpu().numpy(), r["loss"], r["b_loss"])
    lse_in = None if k["kind"] == "bce" else _t(r["lse32"])
    outs = {}
    small = D.geometry(k["name"])[0]
    for cc in (small, 0):
        outs[cc] = _bwd(eng, T, k, lse_in, cc)
        for nm, got, want, bound in zip(("g_a", "g_p", "g_tgt"), outs[cc], r["want"], r["bound"]):
            _inside(f"{tag} {nm} chunk {cc}", got.cpu().numpy(), want, bound)
    assert torch.equal(outs[small][2], outs[0][2]), "g_tgt differs between the smallest chunk width and the default"


@pytest.mark.parametrize("fam", ["dist", "f32"])
def test_guards_around_gradients_and_workspace(eng, fam):
    """The three gradient outputs and the workspace between sentinel margins (the pattern of
    test_gpu_ce_dist.test_guards_and_workspace_tail_are_untouched), on a walked ce case of either family at the smallest
    chunk width."""
    from kge_amd import _lib
    idx = next(i for i, c in enumerate(D.CASES) if D.is_walk(c) and c["kind"] == "ce" and (c["name"] in D.F32) == (fam == "f32")
               and c.get("g_scalar") is None)
    direction = D.directions(D.CASES[idx])[0]
    r = _ref(idx, direction)
    k = r["k"]
    n, E, d = k["n"], k["E"], k["d"]
    dr = k["rel"].shape[1]
    T = _tables(eng, k)
    lib, tc, keep = _lib.lib(), T.c(), []
    ix = [eng._index(_t(x), T.device, keep) for x in (k["a"], k["p"], k["label"])]
    wsb, fwd, bwd = (getattr(lib, f"kge_ce_{fam}_{x}") for x in ("workspace_bytes", "fwd", "bwd"))
    need = wsb(ctypes.byref(tc), n, D.geometry(k["name"])[0])
    assert need > 0 and need % 256 == 0
    S = 7.25
    ws = torch.full((4096 + need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    rows = torch.full((2, n + 2), S, device=DEV)
    ga, gp, gt = (torch.full((r_ + 2, w), S, device=DEV) for r_, w in ((n, d), (n, dr), (E, d)))
    st = eng._stream(T.device)
    dirc = _lib.SP_ if direction == "sp" else _lib.PO_
    g_rows = _t(k["g_rows"])
    wsp = ws.data_ptr() + 4096
    assert wsp % 256 == 0
    _lib.check(fwd(ctypes.byref(tc), dirc, *ix, n, rows[0, 1:].data_ptr(), rows[1, 1:].data_ptr(), wsp, need, st), "fwd")
    _lib.check(bwd(ctypes.byref(tc), dirc, *ix, n, rows[1, 1:].data_ptr(), g_rows.data_ptr(), 1.0, ga[1:].data_ptr(),
                   gp[1:].data_ptr(), gt[1:].data_ptr(), wsp, need, st), "bwd")
    torch.cuda.synchronize()
    assert bool((ws[:4096] == 0x5A).all()) and bool((ws[4096 + need:] == 0x5A).all()), "workspace margins written"
    assert bool((rows[:, 0] == S).all()) and bool((rows[:, n + 1] == S).all()), "loss_rows / lse guards"
    for nm, x, r_ in (("g_a", ga, n), ("g_p", gp, n), ("g_tgt", gt, E)):
        assert bool((x[0] == S).all()) and bool((x[r_ + 1] == S).all()), nm + " guard rows"
        assert bool(torch.isfinite(x[1:r_ + 1]).all()) and not bool((x[1:r_ + 1] == S).any()), nm + ": not written"
    _inside(f"guards {fam} lse", rows[1, 1:n + 1].cpu().numpy(), r["z"], r["b_lse"])
    _inside(f"guards {fam} loss_rows", rows[0, 1:n + 1].cpu().numpy(), r["loss"], r["b_loss"])
