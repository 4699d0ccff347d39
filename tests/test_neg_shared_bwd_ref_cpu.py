"""tests/_neg_shared_bwd_ref.py checked on the CPU: `samples` against engine.shared_samples, the materialised reference
against its folded second statement and against float64 torch autograd through oracle/torch_port.py on the expanded
triples, the rounding bound against planted defects on the very inputs of tests/test_gpu_neg_shared_bwd.py (a defect must
exceed the bound 8 times over in at least one element), the inputs themselves, and the branch of
run_neg_shared_bwd_accum's launch rules that every case reaches."""
import numpy as np
import pytest
import torch

import torch_port as tp
import _neg_bwd_ref as NB
import _neg_shared_bwd_ref as S

SHARP = 8.0
SMALL = [(name, lp) for name in S.NAMES for lp in ((1.0, 2.0, 3.0) if name in ("transe", "rotate") else (1.0,))]
_MADE = {}


def _made(case, slot):
    """(case inputs, want, bound), made once per (case, slot) and never modified"""
    key = (S.case_id(case), slot)
    if key not in _MADE:
        k = S.make_case(case, slot)
        _MADE[key] = (k,) + tuple(NB.reference(k))
    return _MADE[key]


@pytest.mark.parametrize("case", S.CASES + S.UNSUPPORTED, ids=S.case_id)
def test_samples_are_the_engines(case):
    from kge_amd import engine
    for slot in (0, 2):
        k = _made(case, slot)[0] if case in S.CASES else S.make_case(case, slot)
        want = engine.shared_samples(torch.from_numpy(k["unique"]), None if k["drop"] is None else
                                     torch.from_numpy(k["drop"]), torch.from_numpy(k["repeat"]), k["n"]).numpy()
        assert k["neg"].shape == (k["n"], k["K"]) and np.array_equal(k["neg"], want)
        ph = S.physical(k["drop"], k["repeat"], k["n"], k["Uc"])
        assert np.array_equal(k["unique"][ph], want)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_materialised_and_folded_statements_agree(case):
    for slot in (0, 2):
        k, want, _ = _made(case, slot)
        got = S.shared_bwd_accum(*S.shared_args(k))
        fold = S.shared_bwd_accum_folded(*S.shared_args(k))
        for g, f, w in zip(got, fold, want):
            assert np.array_equal(g, w)  # (the reference of the GPU file is shared_bwd_accum)
            assert np.abs(f - w).max() <= 1e-12 * np.abs(w).max()


def _autograd(k):
    ent = torch.tensor(k["ent"], dtype=torch.float64, requires_grad=True)
    rel = torch.tensor(k["rel"], dtype=torch.float64, requires_grad=True)
    Sx, Px, Ox = NB.triples_of(k)
    sc = tp.score_spo(k["name"], ent, rel, torch.tensor(Sx), torch.tensor(Px), torch.tensor(Ox), k["l_norm"])
    (sc * torch.tensor(np.asarray(k["gout"], np.float64).reshape(-1))).sum().backward()
    return ent.grad.numpy(), rel.grad.numpy()


@pytest.mark.parametrize("name,lp", SMALL, ids=[f"{n}-L{l:g}" for n, l in SMALL])
@pytest.mark.parametrize("slot", [0, 2])
@pytest.mark.parametrize("samp", ["naive", "default"])
def test_reference_matches_float64_autograd(name, lp, slot, samp):
    """shared_bwd_accum == autograd of torch_port.score_spo on the n K expanded triples in float64 (1e-12 of the largest
    gradient), on top of pre-loaded tables, with drops and repeats; so is the folded statement."""
    k = S.make_case(S._c(name, lp, 5, 6, 6, samp, pitched=True, nrep=3), slot, seed=23 + slot)
    if name == "transe":
        assert NB.transe_ties(k) > 0
    auto = _autograd(k)
    for fn in (S.shared_bwd_accum, S.shared_bwd_accum_folded):
        for got, want, init in zip(fn(*S.shared_args(k)), auto, (k["ge0"], k["gr0"])):
            assert np.abs(got - init - want).max() <= 1e-12 * np.abs(want).max()


def _ratio(bad, want, bound):
    """the largest |defective - reference| / bound over both tables (an element with bound 0 that moved: infinite)"""
    worst = 0.0
    for b, w, bd in zip(bad, want, bound):
        err = np.abs(b - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bd, 0.0)
        worst = max(worst, float(r.max()) if r.size else 0.0)
    return worst


def _defects(k):
    """(label, "m" -- a defect of the materialised statement -- or "f" -- of the folded one --, defect)"""
    n, P, uc, K, slot = k["n"], k["P"], k["Uc"], k["K"], k["slot"]
    drop, rep = k["drop"], k["repeat"]
    nc = S.shared_nc(k["d"])
    t0, t1 = S.role0_tile(nc), S.role1_tile(nc)
    ph = S.physical(drop, rep, n, uc)
    W = S.fold_weights(drop, rep, k["gout"], n, uc)
    feats = S.fold_features(k)
    fixed, vary = ("o", "s") if slot == 0 else ("s", "o")
    # the last physical row of the first ROLE 0 tile with a weight, and the last positive that weighs it
    u = max(x for x in range(min(t0, P)) if (W[:, x] != 0).any())
    i = max(x for x in range(n) if W[x, u] != 0)
    cols = lambda r, rows: r * K + np.flatnonzero(np.isin(ph[r], rows))
    out = [("one pair dropped", "m", dict(drop=("spo", cols(i, [u])))),
           ("a ROLE 0 flush dropped", "m", dict(drop=(fixed + "p", cols(n - 1, np.arange(t0))))),
           ("a ROLE 1 flush dropped", "m", dict(drop=(vary, np.concatenate([cols(r, [u]) for r in range(min(t1, n))])))),
           ("last coordinate zero", "m", dict(zero_last=vary))]
    if drop is not None and (drop < uc).any():
        out.append(("drop rule ignored in the base fold", "f", dict(base_ignores_drop=True)))
    if "repeat_of_dropped" in feats:
        out.append(("drop rule ignored in the repeat fold", "f", dict(repeat_ignores_drop=True)))
    if rep.size:
        out.append(("repeat columns left out", "f", dict(no_repeats=True)))
    if "dup_repeat" in feats:
        out.append(("a duplicated repeat counted once", "f", dict(dup_once=True)))
    if k["l_norm"] == 2.0 and drop is not None and ((drop > 0) & (drop < uc)).any():
        out.append(("the spare's distance from column 0", "f", dict(spare_dist_col0=True)))
    if k["name"] != "distmult":  # (s r o is symmetric in s and o)
        out.append(("slots swapped", "m", dict(swap_slots=True)))
    if n > 1:
        out.append(("next row's relation", "m", dict(rel_next=K)))
    if k["name"] == "complex":
        out.append(("cross term sign", "m", dict(flip_cross=True)))
    if k["name"] == "transe" and k["l_norm"] == 1.0 and NB.transe_ties(k) > 0:
        out.append(("epsilon left out at the ties", "m", dict(eps=0.0)))
    if k["preloaded"]:
        out.append(("pre-loaded gradient overwritten", "m", dict(overwrite=True)))
    return out


def _well_posed(k):
    if k["name"] == "transe":  # the grid (planted ties reach 4): differences exact in float32 and float64 alike
        for x in (k["ent"], k["rel"]):
            assert (np.abs(x) <= 4.0).all() and (x * 64 == np.round(x * 64)).all()
        assert NB.transe_ties(k) > 0 or k["d"] == 1
    if k["name"] == "rotate":
        assert NB.rotate_min_modulus(k) >= 2.0 ** -6
    assert (np.abs(k["gout"]) >= 0.5).all() and (np.abs(k["gout"]) <= 1.0).all()
    for x in (k["ge0"], k["gr0"]):
        assert not (np.signbit(x) & (x == 0)).any()  # no -0.0: the kernel's +0.f flush would change its bits
    assert 0 <= k["unique"].min() and k["unique"].max() < k["E"]
    assert k["drop"] is None or (0 <= k["drop"].min() and k["drop"].max() <= k["Uc"])
    assert k["repeat"].size == 0 or (0 <= k["repeat"].min() and k["repeat"].max() < k["Uc"])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_bound_is_sharp_and_inputs_well_posed(case):
    for slot in (0, 2):
        k, want, bound = _made(case, slot)
        _well_posed(k)
        for w, b, bb in zip(want, bound, S.shared_bwd_accum_bound(*S.shared_args(k))):
            assert np.isfinite(w).all() and np.isfinite(b).all() and (b >= 0).all() and np.array_equal(b, bb)
        for label, form, defect in _defects(k):
            if form == "m":
                bad = NB.neg_bwd_accum(*NB.ref_args(k), defect=defect)
            else:
                bad = S.shared_bwd_accum_folded(*S.shared_args(k), defect=defect)
            ratio = _ratio(bad, want, bound)
            assert ratio >= SHARP, (S.case_id(case), slot, label, ratio)


def test_every_defect_is_planted_somewhere():
    labels = set()
    for c in S.CASES:
        labels |= {label for label, _, _ in _defects(_made(c, 2)[0])}
    assert len(labels) == 14, sorted(labels)


def test_reduction_lengths_stay_short():
    """every table element of every case sums about 700 terms or fewer (780: 41 columns of one physical row for 19
    positives): up to there one dropped pair must show 8 times over"""
    for c in S.CASES:
        for slot in (0, 2):
            k = _made(c, slot)[0]
            Sx, Px, Ox = NB.triples_of(k)
            ke = np.bincount(Sx, minlength=k["E"]) + np.bincount(Ox, minlength=k["E"])
            assert ke.max() <= 780 and np.bincount(Px).max() <= 700, (S.case_id(c), slot, ke.max(), np.bincount(Px).max())
            if k["l_norm"] != 1.0 and not k.get("pitched"):
                assert ke.max() <= 48 and k["d"] <= 130


def test_the_cancelling_pair_is_shown_and_weighs_zero():
    for c in (c for c in S.CASES if c.get("fold") == "cancel"):
        for slot in (0, 2):
            k = _made(c, slot)[0]
            W = S.fold_weights(k["drop"], k["repeat"], k["gout"], k["n"], k["Uc"])
            ph = S.physical(k["drop"], k["repeat"], k["n"], k["Uc"])
            for i in range(k["n"]):
                u = k["Uc"] if k["drop"][i] == 9 else 9
                assert W[i, u] == 0.0 and (ph[i] == u).sum() == 2
            assert (k["drop"] == 9).any() and (k["drop"] != 9).any()


# ---- the launch rules and the branch each case reaches ---------------------------------------------------------------------
def test_launch_rules():
    assert [S.shared_nc(d) for d in (1, 2, 128, 129, 130, 256, 257, 258, 512, 513, 514, 1023, 1024, 1025, 1026)] == \
        [1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8, 8, None, None]
    assert [S.role0_tile(nc) for nc in (1, 2, 4, 8)] == [64, 32, 16, 8]
    assert [S.role1_tile(nc) for nc in (1, 2, 4, 8)] == [32, 16, 8, 4]
    assert (S.OWNERS_PER_WG, S.OWNERS_PER_WAVE, S.STAGE_FLOATS) == (16, 4, 8192)


# (n, P, d) -> facts of `branches` the shape was chosen for
BRANCHES = {
    (1, 1, 1): dict(nc=1, r0_tiles=1, r0_last=1, r1_tiles=1, r1_last=1, r0_wgs=1, r0_owners_last=1, r1_owners_last=1),
    (1, 2, 1): dict(nc=1, r0_tiles=1, r0_last=2, r1_last=1, r0_owners_last=1, r1_owners_last=2, odd=True),
    (1, 1, 2): dict(nc=1, r0_last=1, r1_last=1, r1_owners_last=1),
    (1, 2, 2): dict(nc=1, r0_last=2, r1_last=1, r1_owners_last=2),
    (33, 65, 128): dict(nc=1, r0_tiles=2, r0_last=1, r1_tiles=2, r1_last=1, r0_wgs=3, r0_owners_last=1, r1_wgs=5,
                        r1_owners_last=1, full0=True),
    (17, 33, 130): dict(nc=2, r0_tiles=2, r0_last=1, r1_tiles=2, r1_last=1, r0_wgs=2, r0_owners_last=1, r1_wgs=3,
                        r1_owners_last=1, full0=False),
    (17, 33, 256): dict(nc=2, r0_tiles=2, r0_last=1, r1_tiles=2, r1_last=1, full0=True, full1=True),
    (5, 9, 514): dict(nc=8, r0_tiles=2, r0_last=1, r1_tiles=2, r1_last=1, full0=False),
    (5, 9, 1024): dict(nc=8, r0_tiles=2, r0_last=1, r1_tiles=2, r1_last=1, r0_wgs=1, r0_owners_last=5, r1_owners_last=9,
                       full0=True),
    (5, 9, 1023): dict(nc=8, r0_tiles=2, r0_last=1, r1_tiles=2, r1_last=1, odd=True, full0=False),
    (300, 5, 40): dict(nc=1, r0_tiles=1, r0_last=5, r1_tiles=10, r1_last=12, r0_wgs=19, r0_owners_last=12, r1_wgs=1,
                       r1_owners_last=5),
    (300, 6, 40): dict(nc=1, r0_last=6, r1_tiles=10, r1_last=12, r1_wgs=1, r1_owners_last=6),
    (5, 8, 2): dict(nc=1, r0_tiles=1, r0_last=8, r1_tiles=1, r1_last=5), (5, 8, 33): dict(nc=1, r0_last=8, odd=True),
    (5, 8, 66): dict(nc=1, r0_last=8), (5, 8, 130): dict(nc=2, r0_tiles=1, r0_last=8, r1_tiles=1, r1_last=5),
}
for _d in (40, 33):  # nc = 1 at the owner and tile edges; the fold and pitched cases
    for _n, (_w, _o) in ((15, (1, 15)), (16, (1, 16)), (17, (2, 1))):
        for _P, (_t, _l), (_w1, _o1) in ((63, (1, 63), (4, 15)), (64, (1, 64), (4, 16)), (65, (2, 1), (5, 1))):
            BRANCHES[(_n, _P, _d)] = dict(nc=1, r0_tiles=_t, r0_last=_l, r1_tiles=1, r1_last=_n, r0_wgs=_w,
                                          r0_owners_last=_o, r1_wgs=_w1, r1_owners_last=_o1, full0=False, odd=bool(_d % 2))
    for _P in (70, 71):
        BRANCHES[(19, _P, _d)] = dict(nc=1, r0_tiles=2, r0_last=_P - 64, r1_tiles=1, r1_last=19, r0_wgs=2,
                                      r0_owners_last=3, r1_wgs=5, r1_owners_last=_P - 64)
for _d in (258, 400, 512):  # nc = 4
    for _n, (_t1, _l1) in ((7, (1, 7)), (8, (1, 8)), (9, (2, 1))):
        for _P, (_t, _l), (_w1, _o1) in ((15, (1, 15), (1, 15)), (16, (1, 16), (1, 16)), (17, (2, 1), (2, 1))):
            BRANCHES[(_n, _P, _d)] = dict(nc=4, r0_tiles=_t, r0_last=_l, r1_tiles=_t1, r1_last=_l1, r0_wgs=1,
                                          r0_owners_last=_n, r1_wgs=_w1, r1_owners_last=_o1,
                                          full0=(_d == 512 and _P >= 16))


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_cases_reach_their_branches(case):
    for slot in (0, 2):
        k = _made(case, slot)[0]
        got = S.branches(k)
        for name, value in BRANCHES[(k["n"], k["P"], k["d"])].items():
            assert got[name] == value, (S.case_id(case), slot, name, got)
        if case.get("fold"):
            assert case["fold"] in got["fold"], (S.case_id(case), slot, got["fold"])


def test_every_branch_has_a_case():
    """every nc; for each role a last tile of one and a full last tile (behind at least one other tile for the tile of
    one); owner workgroups of 1 and of 16 owners; the staging buffer full at nc = 1 and nc = 8 (and at 2 and 4), in
    ROLE 1 too (entity and relation rows side by side); odd d under nc = 1 and nc = 8; every fold feature; l_norm 2 and 3
    for both distance scorers at d = 2, 33 / 66, 130 with drop and repeats; pitched and pre-loaded cases with a `scores`
    slice; both sampling kinds on every shape."""
    cb = [(c, S.branches(_made(c, 0)[0])) for c in S.CASES]
    assert {b["nc"] for _, b in cb} == {1, 2, 4, 8}
    for nc in (1, 2, 4, 8):
        assert any(b["nc"] == nc and b["r0_tiles"] > 1 and b["r0_last"] == 1 for _, b in cb)
        assert any(b["nc"] == nc and b["r1_tiles"] > 1 and b["r1_last"] == 1 for _, b in cb)
    for nc in (1, 4):
        assert any(b["nc"] == nc and b["r0_last"] == S.role0_tile(nc) for _, b in cb)
    assert any(b["nc"] == 4 and b["r1_last"] == S.role1_tile(4) for _, b in cb)
    for role in ("r0", "r1"):
        assert any(b[role + "_wgs"] > 1 and b[role + "_owners_last"] == 1 for _, b in cb)
        assert any(b[role + "_owners_last"] == S.OWNERS_PER_WG for _, b in cb)
    assert {b["nc"] for _, b in cb if b["full0"]} == {1, 2, 4, 8}
    assert {b["nc"] for _, b in cb if b["full1"]} >= {1, 8}
    assert any(b["odd"] and b["nc"] == 1 for _, b in cb) and any(b["odd"] and b["nc"] == 8 for _, b in cb)
    feats = set().union(*(b["fold"] for _, b in cb))
    assert feats >= set(S.FOLDS), set(S.FOLDS) - feats
    assert all(S.shared_nc(c["d"]) is None for c in S.UNSUPPORTED) and {c["d"] for c in S.UNSUPPORTED} == {1025, 1026}
    for name, dmid in (("transe", 33), ("rotate", 66)):
        for lp in (2.0, 3.0):
            cs = [c for c in S.CASES if c["name"] == name and c["l_norm"] == lp and not c.get("pitched")]
            assert {c["d"] for c in cs} == {2, dmid, 130} and all(c["samp"] == "default" and c["nrep"] for c in cs)
    assert any(c.get("pitched") and c["l_norm"] == 2.0 for c in S.CASES)
    assert any(c.get("pitched") and c["name"] == "complex" for c in S.CASES)
    shapes = lambda samp: {(c["n"], c["Uc"] + (samp == "default"), c["d"], c["name"]) for c in S.CASES
                           if c["samp"] == samp and not c.get("fold") and c["l_norm"] == 1.0 and c["n"] > 1
                           and c["n"] != 300 and not c.get("pitched")}
    assert shapes("naive") == shapes("default")
