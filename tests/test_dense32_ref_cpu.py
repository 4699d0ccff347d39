"""tests/_dense32_ref.py checked without a GPU, on the very inputs tests/test_gpu_dense32_bound.py runs: the float64
reference against float64 autograd of the reference op sequence (oracle/torch_port.py + cross_entropy, the composed kl and
bce), every planted property of the case list, the float32 restatements of the forward and of the `weight` lambda inside
the bounds, and PLANTED DEFECTS that must exceed the bounds 8 times over (the factor of test_pairs_bwd16_ref_cpu.py) on
every case they apply to.  The score bits are the oracle's (what kge_score_sp / kge_score_po store).

Nothing here or in _dense32_ref.py was fitted to a kernel's output: the conditions below are conditions on the inputs."""
import numpy as np
import pytest
import torch

import torch_port as tp
import _dense32_ref as D

FACTOR = 8.0
_K = {}


def _case(case, direction):
    key = (D.case_id(case), direction)
    if key not in _K:
        k = D.make_case(case, direction)
        x32 = D.oracle_scores(k)
        lse32 = D.ref_lse32(x32)
        P, e = D.coef64(k, x32, lse32), D.coef_radius(k, x32, lse32)
        want, bound = D.grads_and_bound(k, P, e)
        loss, z = D.loss64(k, x32)
        _K[key] = dict(k=k, x32=x32, lse32=lse32, P=P, e=e, want=want, bound=bound, loss=loss, z=z,
                       b_loss=D.loss_bound(k, x32), b_lse=D.lse_bound(x32, k["n"], k["name"]))
    return _K[key]


ALL = [(c, d) for c in D.CASES for d in D.directions(c)]
IDS = [f"{D.case_id(c)}-{d}" for c, d in ALL]
# (every case that is not walked, and one walked case: the closed forms do not depend on the shape)
SMALL = [(c, d) for c, d in ALL if not D.is_walk(c) or (c["kind"] == "ce" and c["name"] in ("transe", "complex"))]


# ---- the reference against float64 autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("case,direction", SMALL, ids=[f"{D.case_id(c)}-{d}" for c, d in SMALL])
def test_reference_matches_float64_autograd(case, direction):
    """losses and gradients of the reference, fed with the float64 scores of the op sequence, == autograd (1e-12)"""
    k = D.make_case(case, direction)
    n, E = k["n"], k["E"]
    ent = torch.tensor(k["ent"], dtype=torch.float64, requires_grad=True)
    rel = torch.tensor(k["rel"], dtype=torch.float64, requires_grad=True)
    a, p = torch.tensor(k["a"]), torch.tensor(k["p"])
    sc = tp.score_sp(k["name"], ent, rel, a, p, None, k["l_norm"]) if direction == "sp" else \
        tp.score_po(k["name"], ent, rel, p, a, None, k["l_norm"])
    y = torch.tensor(D.label_matrix(k, E).astype(np.float64))
    if k["kind"] == "ce":
        rows = torch.nn.functional.cross_entropy(sc, torch.tensor(k["label"]), reduction="none")
    elif k["kind"] == "bce":
        rows = tp.bce_loss(sc, y, k["offset"], reduction="rows")
    elif k.get("label_weight") is not None:
        rows = torch.logsumexp(sc, 1) - torch.tensor(k["label_weight"].astype(np.float64)) * (sc * y).sum(1)
        if k.get("label_bias") is not None:  # the loss rows carry no bias (kge_kl_f32_fwd has none): compared first
            assert np.allclose(D.loss64(k, sc.detach().numpy())[0], rows.detach().numpy(), rtol=1e-12, atol=1e-11)
            rows = rows - torch.tensor(k["label_bias"].astype(np.float64)) * sc.sum(1)  # label smoothing's uniform term
    else:
        # tp.kl_loss's functions with the labels kept in float64 (kl_loss normalises them in float32)
        F = torch.nn.functional
        rows = torch.nn.KLDivLoss(reduction="none")(F.log_softmax(sc, dim=1), F.normalize(y, p=1, dim=1)).sum(dim=1)
    g = np.full(n, np.float32(k["g_scalar"]), np.float32) if k.get("g_rows") is None else k["g_rows"]
    (rows * torch.tensor(g.astype(np.float64))).sum().backward()
    x = sc.detach().numpy()
    loss, z = D.loss64(k, x)
    assert k.get("label_bias") is not None or np.allclose(loss, rows.detach().numpy(), rtol=1e-12, atol=1e-11)
    assert np.isfinite(ent.grad.numpy()).all() and np.isfinite(rel.grad.numpy()).all()
    w = None
    if k["kind"] == "kl" and k.get("label_weight") is None:
        w = 1.0 / np.maximum(np.diff(k["rowptr"]), 1)  # (row_gradients holds fl32(1 / k_i), what the kernel multiplies by)
    P = D.coef64(k, x, z if z is not None else np.zeros(n), w)  # the exact lse: the coefficient autograd forms
    g_a, g_p, g_t = D.grads(k, P)
    ge = g_t.copy()
    np.add.at(ge, k["a"], g_a)
    gr = np.zeros(k["rel"].shape)
    np.add.at(gr, k["p"], g_p)
    for got, want in ((ge, ent.grad.numpy()), (gr, rel.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ---- planted properties --------------------------------------------------------------------------------------------------
def test_walk_geometry_and_case_list():
    d, E, n = D.WALK_DIST
    assert E == 64 * 513 + 1 and D.cd_groups(n, E) == (3, 172) and -(-E // 64) == 514
    assert 171 * 3 * 64 == E - 1  # the short last group: one tile, one valid column
    assert D.records_bytes(n, E) not in (-(-(n * g * 12) // 256) * 256 for g in (171, 173))
    assert D.cd_groups(256, 16384) == (1, 256) and D.cd_groups(256, 16385)[0] == 2  # the threshold of the issue
    cols = D.walk_label_cols(n, E)
    assert [c // 64 // 3 for c in cols] == [0, 0, 86, 86, 170, 170, 171] and [c // 64 % 3 for c in cols[:6]] == [1, 2] * 3
    walk = [c for c in D.CASES_DIST if D.is_walk(c)]
    for name in ("transe", "rotate"):
        assert {c["kind"][:2] for c in walk if c["name"] == name} == {"ce", "kl", "bc"}
    assert {(c["name"], c["l_norm"]) for c in D.CASES_DIST} == {(s, l) for s in ("transe", "rotate") for l in (1.0, 2.0)}
    assert {(c["d"], c["E"], c["n"]) for c in D.CASES_DIST} == {D.GEO, D.FULL, D.ONE, D.RAG1, D.ODD, D.WALK_DIST}
    assert {c["profile"] for c in D.CASES_DIST} == {"ascending", "descending", "spike_first", "spike_last", "spike_tile2",
                                                    "plateau", "zero"}
    assert {c["profile"] for c in D.CASES_DIST if c["name"] == "transe" and c["l_norm"] == 1.0} >= {"zero"}
    for kind in ("ce", "kl", "bce"):
        assert sum(1 for c in D.CASES_DIST if c["kind"][:2] == kind[:2] and c.get("g_scalar") is not None) >= 1
    assert all(c["why"] for c in D.CASES)


def test_walk_geometry_and_case_list_f32():
    d, E, n, ld = D.WALK_F32
    assert E == 128 * 300 + 1 and D.cf_groups(n, E) == (2, 151) and -(-E // 128) == 301 and 150 * 2 * 128 == E - 1
    assert D.cf_groups(256, 128 * 256) == (1, 256) and D.cf_groups(256, 128 * 256 + 1)[0] == 2
    assert D.geometry("complex") == (128, 2, 4) and D.geometry("rotate") == (64, 4, 1)
    cols = D.walk_label_cols(n, E, "complex")
    assert [c // 128 // 2 for c in cols] == [0, 75, 149, 150] and [c // 128 % 2 for c in cols[:3]] == [1, 1, 1]
    walk = [c for c in D.CASES_F32 if D.is_walk(c)]
    for name in D.F32:
        assert {c["kind"][:2] for c in walk if c["name"] == name} == {"ce", "kl", "bc"}
    assert {(c["d"], c["E"], c["n"], c["ent_ld"]) for c in D.CASES_F32} == {D.F_RAG, D.F_FULL, D.F_ONE, D.F_LD, D.F_BIG, D.WALK_F32}
    assert any(c["ent_ld"] > c["d"] for c in D.CASES_F32) and any(c["kind"] == "klwb" for c in D.CASES_F32)
    assert {c["profile"] for c in D.CASES_F32} == {"ascending", "descending", "spike_first", "spike_last", "spike_tile2",
                                                   "plateau"}
    for kind in ("ce", "kl", "bce"):
        assert sum(1 for c in D.CASES_F32 if c["kind"][:2] == kind[:2] and c.get("g_scalar") is not None) >= 1


@pytest.mark.parametrize("case,direction", ALL, ids=IDS)
def test_planted_properties(case, direction):
    r = _case(case, direction)
    k, x = r["k"], r["x32"].astype(np.float64)
    n, m, prof, hot = k["n"], k["E"], case["profile"], k["hot"]
    T, G = D.groups(k["name"], n, m)
    tw, nt, spt = D.geometry(k["name"])
    f32 = k["name"] in D.F32
    xs = x[k["hot_rows"]]
    if k["name"] == "transe":  # q and q - t exact in float32: the grid, and magnitudes far below 2^24 grid steps
        q = k["ent"][k["a"]].astype(np.float64) + (1 if direction == "sp" else -1) * k["rel"][k["p"]].astype(np.float64)
        assert np.array_equal(q, q.astype(np.float32)) and np.array_equal(q * 64, np.round(q * 64))
        assert np.abs(q).max() + np.abs(k["ent"]).max() < 2.0 ** 12
        if k["l_norm"] == 1.0:  # an exactly representable sum: the oracle's L1 bits are the exact distance
            assert np.array_equal(-xs[0], np.abs(q[k["hot_rows"][0]][None, :] - k["ent"].astype(np.float64)).sum(1))
    if f32:
        assert prof in ("ascending", "descending") or (np.abs(xs).max(axis=1) >= 100).all()
        assert (k["rel"][0] == np.r_[np.ones(k["d"] // (2 if k["name"] == "complex" else 1)),
                                     np.zeros(k["d"] // 2 if k["name"] == "complex" else 0)]).all()
    elif prof != "zero":
        assert (np.abs(xs) >= 100).all()
        assert (r["x32"] < 0).all()
    mx = xs.argmax(axis=1)
    if prof in ("spike_first", "spike_last", "spike_tile2", "plateau"):
        assert np.isin(mx, hot).all()
        assert (xs.max(axis=1)[:, None] - np.delete(xs, hot, axis=1) > 104).all()  # every other term flushes
        grp = np.arange(m) // tw // T
        other = [g for g in range(G) if g != hot[0] // tw // T]
        assert G == 1 or all((xs.max(axis=1)[:, None] - xs[:, grp == g] > 104).all() for g in other)  # whole groups
    if prof == "spike_last":
        assert hot[0] == m - 1 and 1 <= m % tw <= tw - tw // nt  # inside the ragged tile, behind an all-padding thread
    if prof == "spike_tile2":
        assert T > 1 and hot[0] // tw % T == 1
    if prof == "plateau":
        assert (k["ent"][hot] == k["ent"][hot[0]]).all() and hot.size == 5
        assert (r["x32"][k["hot_rows"]][:, hot] == r["x32"][k["hot_rows"]][:, hot[:1]]).all()
        assert np.allclose(D.lse64(xs), xs[:, hot[0]] + np.log(5), rtol=0, atol=1e-12)
    if prof in ("ascending", "descending") and f32:
        # a thread folds 16-column blocks in ascending column order: the block maxima move at every block
        nblk = -(-m // 16)
        pad = np.full((xs.shape[0], nblk * 16), -np.inf)
        pad[:, :m] = xs
        step = np.diff(pad.reshape(xs.shape[0], nblk, 16).max(axis=-1), axis=1)
        assert (step > 0).all() if prof == "ascending" else (step < 0).all()
        assert (mx // 16 == (nblk - 1 if prof == "ascending" else 0)).all()
    elif prof in ("ascending", "descending"):
        # per fold thread (row, 16-column slot fq): its maximum over tile t, for every tile that has the slot
        tiles = -(-m // 64)
        pad = np.full((xs.shape[0], tiles * 64), -np.inf)
        pad[:, :m] = xs
        tm = pad.reshape(xs.shape[0], tiles, 4, 16).max(axis=-1)
        step = np.diff(tm, axis=1)
        live = np.isfinite(tm[:, 1:]) & np.isfinite(tm[:, :-1])
        assert live.any() or tiles == 1
        assert (step[live] > 0).all() if prof == "ascending" else (step[live] < 0).all()
        assert (mx // 64 == (tiles - 1 if prof == "ascending" else 0)).all()
    if prof == "zero":
        assert (r["x32"][k["hot_rows"], hot[0]] == 0).all() and (mx == hot[0]).all() and k["zero_pairs"].sum() == len(xs)
        A, Rr = k["ent"][k["a_hot"]], k["rel"][0]
        assert (Rr == 0).all() and (k["ent"][hot[0]] == A).all()
        if k["kind"] == "ce":  # once on the label column, once off it
            lab = k["label"][k["hot_rows"]]
            assert (lab == hot[0]).any() and (lab != hot[0]).any()
    elif k["name"] == "rotate":
        assert R_min_modulus(k) > 0.02
    if k["kind"] == "ce":
        lab = k["label"]
        if n >= 16:
            assert {c for c in D.LABEL_COLS + (m - 1,) if c < m} <= set(lab.tolist())
            assert np.unique(lab).size < n and hot[0] in lab[k["hot_rows"]] and (lab[k["hot_rows"]] != hot[0]).any()
        if T > 1:
            assert set(D.walk_label_cols(n, m, k["name"])) <= set(lab.tolist())
    else:
        cnt = np.diff(k["rowptr"])
        rows = D.csr_rows(k)
        assert all(len(set(js.tolist())) == len(js) for js in rows)
        if n > 4:
            assert (cnt == 0).any() and (cnt == 1).any() and (cnt == min(65, m)).any() and (cnt == m).any()
            assert {c for c in (0, 31, 32, 63, 64, 127, 128, m - 1) if c < m} <= set(k["col"].tolist())
        else:
            assert cnt[0] == m
    g, _ = D.row_gradients(k)
    if k.get("g_rows") is not None and n >= 8:
        nz = np.abs(k["g_rows"][k["g_rows"] != 0])
        assert (k["g_rows"] == 0).any() and (k["g_rows"] < 0).any() and nz.max() / nz.min() >= 2.0 ** 20
        assert (g[k["hot_rows"][:2]] != 0).all() or k["kind"] == "kl"
    if k["kind"] == "kl" and k.get("label_weight") is None and n > 4:
        assert (g[np.diff(k["rowptr"]) == 0] == 0).all()


def R_min_modulus(k):
    return D.R.rotate_min_modulus(k["direction"], k["ent"], k["rel"], k["a"], k["p"], None, np.ones((k["n"], k["E"])))


# ---- the float32 restatements inside the bounds ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,direction", ALL, ids=IDS)
def test_restatements_lie_inside_the_bounds(case, direction):
    r = _case(case, direction)
    k = r["k"]
    P32 = D.coef_restated(k, r["x32"], r["lse32"]).astype(np.float64)
    assert (np.abs(P32 - r["P"]) <= r["e"]).all()
    loss, z = D.fwd_restated(k, r["x32"])
    assert (np.abs(loss.astype(np.float64) - r["loss"]) <= r["b_loss"]).all()
    if z is not None:
        assert (np.abs(z.astype(np.float64) - r["z"]) <= r["b_lse"]).all()
    if not D.is_walk(case):  # the float32 closed forms on the float32 coefficients: one more evaluation the bound holds for
        got = D.R.pairs_bwd(*D._args(k, P32.astype(np.float32)), dtype=np.float32)
        for g_, w, b in zip(got, r["want"], r["bound"]):
            assert (np.abs(g_ - w) <= b).all()


# ---- planted defects ------------------------------------------------------------------------------------------------------
def _kl(k):
    return k["kind"] == "kl"


def _ragged_pad_thread(k):
    tw, nt, _ = D.geometry(k["name"])
    return 1 <= k["E"] % tw <= tw - tw // nt


def _tw(k):
    return D.geometry(k["name"])[0]


FWD_DEFECTS = {
    # (f32: a spike in the second walked tile sits in a later 16-column step of it, so the factor at the tile's first step
    # is 1 there -- no_rescale_step is the defect that sees it)
    "no_rescale_walk": lambda c, k: D.is_walk(c) and k["kind"] != "bce" and (
        c["profile"] == "ascending" or (c["profile"] == "spike_tile2" and k["name"] not in D.F32)),
    # (a lone spiked row: every factor of the lane merge is exactly 1 or 0 -- nothing to drop)
    "no_rescale_lane": lambda c, k: k["kind"] != "bce" and k["n"] > 1,
    # (f32: every fold step of a thread after its first -- the issue's "dropped at a fold step"; the distance family has one
    # step per walked tile, where no_rescale_walk is that defect)
    "no_rescale_step": lambda c, k: k["name"] in D.F32 and k["kind"] != "bce" and c["profile"] in ("ascending", "spike_tile2"),
    "no_pad": lambda c, k: k["E"] % _tw(k) != 0 and c["profile"] in ("ascending", "spike_last"),
    # (distance family only: its row maxima are negative, so a thread merged as (max 0, sum 0) moves the maximum to 0 and
    # the terms flush; the planted f32 rows have positive maxima, where that merge changes nothing)
    "pad_00": lambda c, k: k["name"] not in D.F32 and k["kind"] != "bce" and _ragged_pad_thread(k) and c["profile"] in ("ascending", "spike_last"),
    "label_group": lambda c, k: D.is_walk(c) and k["kind"] == "ce",
    "no_offset": lambda c, k: k["kind"] == "bce",
}

GRAD_DEFECTS = {
    "label_plus1": lambda c, k: k["kind"] == "ce",
    "g_next": lambda c, k: k["n"] >= 2 and k.get("g_rows") is not None,
    "chunk_last": lambda c, k: True,
    "mask_word": lambda c, k: k["kind"] != "ce",
    "no_w": lambda c, k: _kl(k),
    "no_offset": lambda c, k: k["kind"] == "bce",
    "unlabelled": lambda c, k: _kl(k) and k.get("label_weight") is None and k["n"] > 16,
    "zero_w1": lambda c, k: c["profile"] == "zero",
    "no_bias": lambda c, k: k.get("label_bias") is not None,
    "pad_one": lambda c, k: k["name"] in D.F32 and k["E"] % 128 != 0,
}


FLOOR = 2.0 ** -100  # a bound below this is the subnormal floor of a row with g_i = 0: such elements are left out


def _ratio(err, bound):
    """the largest err / bound over the elements whose bound is above the subnormal floor"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where((err == 0) | (bound <= FLOOR), 0.0, err / bound), initial=0.0))


# the number of (case, direction) pairs of D.CASES every defect applies to: a predicate that narrows fails here.  The
# figures follow from CASES_DIST + CASES_F32 and move with them: a new case changes the counts of the defects it meets.
HITS_FWD = {"no_rescale_walk": 5, "no_rescale_step": 7, "no_rescale_lane": 40, "no_pad": 24, "pad_00": 11, "label_group": 4,
            "no_offset": 16}
HITS_GRAD = {"label_plus1": 24, "g_next": 48, "chunk_last": 64, "mask_word": 40, "no_w": 24, "no_offset": 16,
             "unlabelled": 10, "zero_w1": 8, "no_bias": 5, "pad_one": 24}


def test_walk_only_defects_reach_every_walked_case():
    walked = [(c, d) for c, d in ALL if D.is_walk(c)]
    assert len(ALL) == 64 and len(walked) == 12
    for c, d in walked:
        k = D.make_case(c, d)
        assert FWD_DEFECTS["label_group"](c, k) == (k["kind"] == "ce")
        f32, rises = k["name"] in D.F32, k["kind"] != "bce" and c["profile"] != "spike_last"
        assert FWD_DEFECTS["no_rescale_walk"](c, k) == (rises and not (f32 and c["profile"] == "spike_tile2"))
        assert FWD_DEFECTS["no_rescale_step"](c, k) == (rises and f32)


@pytest.mark.parametrize("defect", sorted(FWD_DEFECTS))
def test_planted_forward_defects_exceed_the_bound(defect):
    hit, low = 0, np.inf
    for case, direction in ALL:
        r = _case(case, direction)
        k = r["k"]
        if not FWD_DEFECTS[defect](case, k):
            continue
        loss, z = D.fwd_restated(k, r["x32"], {defect: True})
        ratio = _ratio(np.abs(loss.astype(np.float64) - r["loss"]), r["b_loss"])
        if z is not None and defect != "label_group":
            ratio = max(ratio, _ratio(np.abs(z.astype(np.float64) - r["z"]), r["b_lse"]))
        print(f"dense32 defect {defect} {D.case_id(case)} {direction}: max err / bound {ratio:.3g}")
        assert ratio >= FACTOR, (defect, D.case_id(case), direction, ratio)
        hit, low = hit + 1, min(low, ratio)
    print(f"dense32 defect {defect}: {hit} cases, smallest ratio {low:.3g}")
    assert hit == HITS_FWD[defect]


@pytest.mark.parametrize("defect", sorted(GRAD_DEFECTS))
def test_planted_gradient_defects_exceed_the_bound(defect):
    hit, low = 0, np.inf
    for case, direction in ALL:
        r = _case(case, direction)
        k = r["k"]
        if not GRAD_DEFECTS[defect](case, k):
            continue
        if defect == "zero_w1":
            got = D.grads(k, r["P"], {"zero_w1": True})
            pairs = [(got[2], r["want"][2], r["bound"][2])]
        elif defect == "pad_one":
            got = D.grads(k, r["P"], {"pad_one": True})
            pairs = list(zip(got, r["want"], r["bound"]))
        else:
            P = D.coef_restated(k, r["x32"], r["lse32"], {defect: True}).astype(np.float64)
            dP = P - r["P"]
            if not (np.abs(dP) > r["e"]).any():
                ratio = 0.0
                pairs = []
            else:  # the gradients are linear in the coefficients: push the difference through
                diff = D.grads(k, dP)
                pairs = [(w + d_, w, b) for d_, w, b in zip(diff, r["want"], r["bound"])]
        ratio = max([_ratio(np.abs(g_ - w), b) for g_, w, b in pairs] + [0.0])
        print(f"dense32 defect {defect} {D.case_id(case)} {direction}: max err / bound {ratio:.3g}")
        assert ratio >= FACTOR, (defect, D.case_id(case), direction, ratio)
        hit, low = hit + 1, min(low, ratio)
    print(f"dense32 defect {defect}: {hit} cases, smallest ratio {low:.3g}")
    assert hit == HITS_GRAD[defect]
