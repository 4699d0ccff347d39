"""tests/_neg_bwd_ref.py checked on the CPU: the float64 closed forms against float64 torch autograd through
oracle/torch_port.py on the expanded triples, the rounding bound against planted defects on the very inputs of
tests/test_gpu_neg_bwd.py (a defect must exceed the bound 8 times over in at least one element: the bound is sharp enough
to see it), the inputs themselves, and the branch of bwd.hip's launch rules that every case reaches."""
import numpy as np
import pytest
import torch

import torch_port as tp
import _neg_bwd_ref as R

SHARP = 8.0
SMALL = [(name, lp) for name in ("complex", "distmult", "transe", "rotate")
         for lp in ((1.0, 2.0, 3.0) if name in ("transe", "rotate") else (1.0,))]


def _autograd(k, S, P, O, g):
    ent = torch.tensor(k["ent"], dtype=torch.float64, requires_grad=True)
    rel = torch.tensor(k["rel"], dtype=torch.float64, requires_grad=True)
    sc = tp.score_spo(k["name"], ent, rel, torch.tensor(S), torch.tensor(P), torch.tensor(O), k["l_norm"])
    (sc * torch.tensor(np.asarray(g, np.float64).reshape(-1))).sum().backward()
    return ent.grad.numpy(), rel.grad.numpy()


@pytest.mark.parametrize("name,lp", SMALL, ids=[f"{n}-L{l:g}" for n, l in SMALL])
@pytest.mark.parametrize("slot", [0, 2])
def test_reference_matches_float64_autograd(name, lp, slot):
    """neg_bwd_accum == autograd of torch_port.score_spo on the n K expanded triples in float64 (1e-12 of the largest
    gradient), on top of pre-loaded tables; spo_bwd's rows scattered == spo_bwd_accum == autograd on the positives.  The
    TransE inputs carry exact ties: they weigh sign(+1e-6) = +1, F.pairwise_distance's epsilon."""
    k = R.make_case(R._neg(name, lp, 5, 7, 6, 30, pitched=True), slot, seed=17 + slot)
    if name == "transe":
        assert R.transe_ties(k) > 0
    S, P, O = R.triples_of(k)
    for got, want, init in zip(R.neg_bwd_accum(*R.ref_args(k)), _autograd(k, S, P, O, k["gout"]), (k["ge0"], k["gr0"])):
        assert np.abs(got - init - want).max() <= 1e-12 * np.abs(want).max()
    g = k["gout"][:, 0]
    args = (name, lp, k["ent"], k["rel"], k["s"], k["p"], k["o"], g)
    gs, gp, go = R.spo_bwd(*args)
    ge, gr = np.zeros(k["ent"].shape), np.zeros(k["rel"].shape)
    np.add.at(ge, k["s"], gs)
    np.add.at(ge, k["o"], go)
    np.add.at(gr, k["p"], gp)
    acc = R.spo_bwd_accum(*args, ge, gr)
    for rows, twice, want in zip((ge, gr), acc, _autograd(k, k["s"], k["p"], k["o"], g)):
        assert np.abs(rows - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(twice - 2 * want).max() <= 1e-12 * np.abs(want).max()


def _ratio(bad, want, bound):
    """the largest |defective - reference| / bound over all outputs (an element with bound 0 that moved: infinite)"""
    worst = 0.0
    for b, w, bd in zip(bad, want, bound):
        err = np.abs(b - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bd, 0.0)
        worst = max(worst, float(r.max()) if r.size else 0.0)
    return worst


def _neg_defects(k):
    n, K, slot = k["n"], k["K"], k["slot"]
    ch = R.neg_chunk(n, K)
    fixed, vary = ("o", "s") if slot == 0 else ("s", "o")
    last = (n - 1) * K + min(ch, K) - 1  # the last negative of the first chunk of the last positive
    out = [("one negative dropped", dict(drop=("spo", [last]))),
           ("a chunk's fixed-row flush dropped", dict(drop=(fixed + "p", np.arange((n - 1) * K, last + 1)))),
           ("slots swapped", dict(swap_slots=True)),
           ("last coordinate zero", dict(zero_last=vary))]
    flat = k["neg"].reshape(-1)
    order = np.argsort(flat, kind="stable")
    ends = np.flatnonzero(np.diff(flat[order])) + 1
    if ends.size:  # the last occurrence of the first run credited to the next entity
        out.append(("run boundary", dict(move=(vary, int(order[ends[0] - 1]), int(flat[order[ends[0]]])))))
    if n > 1:
        out.append(("next row's relation", dict(rel_next=K)))
    return out


def _acc_defects(k):
    n = k["n"]
    ch = R.spo_chunk(n)
    c0 = min(1, (n - 1) // ch) * ch  # the second chunk (the first where there is one only)
    js = np.arange(c0, min(n, c0 + ch))
    out = [("one triple dropped", dict(drop=("spo", [int(js[-1])]))),
           ("a chunk's s / p flush dropped", dict(drop=("sp", js))),
           ("last coordinate zero", dict(zero_last="o")),
           ("next row's relation", dict(rel_next=1))]
    ends = np.flatnonzero(np.diff(k["s"])) + 1
    if ends.size:  # the last triple of an s run credited to the next run's entity
        e = ends[min(1, ends.size - 1)]
        out.append(("run boundary", dict(move=("s", int(e - 1), int(k["s"][e])))))
    return out


def _common(k):
    out = []
    if k["name"] == "complex":
        out.append(("cross term sign", dict(flip_cross=True)))
    if k["name"] == "transe" and k["l_norm"] == 1.0 and R.transe_ties(k) > 0:
        out.append(("epsilon left out at the ties", dict(eps=0.0)))  # the ties then weigh sign(0) = 0 instead of +1
    if k.get("preloaded"):
        out.append(("pre-loaded gradient overwritten", dict(overwrite=True)))
    return out


def _well_posed(k):
    if k["name"] == "transe":  # the grid (planted ties reach 4): differences exact in float32 and float64 alike
        for x in (k["ent"], k["rel"]):
            assert (np.abs(x) <= 4.0).all() and (x * 64 == np.round(x * 64)).all()
        assert R.transe_ties(k) > 0 or k["d"] == 1
    if k["name"] == "rotate":
        assert R.rotate_min_modulus(k) >= 2.0 ** -6


@pytest.mark.parametrize("case", R.NEG_CASES, ids=R.case_id)
def test_neg_bound_is_sharp_and_inputs_well_posed(case):
    for slot in (0, 2):
        k = R.make_case(case, slot)
        _well_posed(k)
        args = R.ref_args(k)
        want, bound = R.neg_bwd_accum(*args), R.neg_bwd_accum_bound(*args)
        for w, b in zip(want, bound):
            assert np.isfinite(w).all() and np.isfinite(b).all() and (b >= 0).all()
        flat = k["neg"].reshape(-1)
        if k["K"] >= 3:  # the positive's own entities among its negatives
            fixed, repl = (k["o"][0], k["s"][0]) if slot == 0 else (k["s"][0], k["o"][0])
            assert k["neg"][0, 1] == fixed and k["neg"][0, 2] == repl
        assert 0 <= flat.min() and flat.max() < k["E"]
        for label, defect in _neg_defects(k) + _common(k):
            ratio = _ratio(R.neg_bwd_accum(*args, defect=defect), want, bound)
            assert ratio >= SHARP, (R.case_id(case), slot, label, ratio)


@pytest.mark.parametrize("case", R.ACC_CASES, ids=R.case_id)
def test_acc_bound_is_sharp_and_inputs_well_posed(case):
    k = R.make_case(case)
    _well_posed(k)
    args = R.ref_args(k)
    want, bound = R.spo_bwd_accum(*args), R.spo_bwd_accum_bound(*args)
    for w, b in zip(want, bound):
        assert np.isfinite(w).all() and np.isfinite(b).all() and (b >= 0).all()
    swapped = args[:4] + (k["o"], k["p"], k["s"]) + args[7:]
    if k["name"] != "distmult":  # (s r o is symmetric in s and o: the accumulated tables do not tell the slots apart)
        assert _ratio(R.spo_bwd_accum(*swapped), want, bound) >= SHARP, (R.case_id(case), "slots swapped")
    for label, defect in _acc_defects(k) + _common(k):
        ratio = _ratio(R.spo_bwd_accum(*args, defect=defect), want, bound)
        assert ratio >= SHARP, (R.case_id(case), label, ratio)


@pytest.mark.parametrize("case", R.SPO_CASES, ids=R.case_id)
def test_spo_bound_is_sharp_and_inputs_well_posed(case):
    k = R.make_case(case)
    _well_posed(k)
    args = R.ref_args(k)
    want, bound = R.spo_bwd(*args), R.spo_bwd_bound(*args)
    for w, b in zip(want, bound):
        assert np.isfinite(w).all() and np.isfinite(b).all() and (b > 0).all()
    swapped = args[:4] + (k["o"], k["p"], k["s"]) + args[7:]
    assert _ratio(R.spo_bwd(*swapped), want, bound) >= SHARP, (R.case_id(case), "slots swapped")
    defects = [("last coordinate zero", dict(zero_last="o"))] + [d for d in _common(k) if "overwrite" not in d[1]]
    if k["n"] > 1:
        defects.append(("next row's relation", dict(rel_next=1)))
    for label, defect in defects:
        ratio = _ratio(R.spo_bwd(*args, defect=defect), want, bound)
        assert ratio >= SHARP, (R.case_id(case), label, ratio)
    if k["name"] == "transe" and k["l_norm"] == 1.0 and k["d"] > 1:  # an exact tie weighs +1: ds = dp = -g, do = +g
        gs, gp, go = want
        assert gs[0, 0] == -k["gout"][0] and gp[0, 0] == -k["gout"][0] and go[0, 0] == k["gout"][0]


def test_reduction_lengths_stay_short():
    """every table element of every accumulating case sums about 700 terms or fewer: up to there one dropped term must
    show 8 times over"""
    for c in R.NEG_CASES + R.ACC_CASES:
        for slot in ((0, 2) if c["kind"] == "neg" else (None,)):
            k = R.make_case(c, slot)
            S, P, O = R.triples_of(k)
            ke = np.bincount(S, minlength=k["E"]) + np.bincount(O, minlength=k["E"])
            assert ke.max() <= 760 and np.bincount(P).max() <= 700, (R.case_id(c), slot, ke.max(), np.bincount(P).max())


# ---- the launch rules and the branch each case reaches ---------------------------------------------------------------------
def test_launch_rules():
    assert R.neg_chunk(19, 70) == 4 and R.neg_chunk(37, 131) == 4 and R.neg_chunk(450, 130) == 7
    assert R.neg_chunk(4100, 130) == 64 and R.neg_chunk(8200, 64) == 64 and R.neg_chunk(512, 1000) == 62
    assert R.neg_chunk(5 * 8192, 1) == 5 and R.neg_chunk(63 * 8192, 1) == 63
    assert R.spo_chunk(37) == 1 and R.spo_chunk(3 * 4096 + 5) == 3 and R.spo_chunk(32 * 4096 + 7) == 32
    assert R.spo_chunk(10 ** 7) == 32
    assert [R.sorted_nc(d) for d in (1, 512, 513, 514, 1023, 1024, 1025, 1026)] == [4, 4, 8, 8, 8, 8, None, None]


# n / K / d -> facts of `branches` the shape was chosen for
NEG_BRANCHES = {
    (1, 1, 1): dict(ch=4, cpr=1, last=1, nc=4, sorted_last=1, odd=True),
    (1, 1, 2): dict(ch=4, cpr=1, last=1, nc=4, sorted_last=1),
    (19, 70, 33): dict(ch=4, cpr=18, last=2, nc=4, odd=True),
    (19, 70, 40): dict(ch=4, cpr=18, last=2, nc=4),
    (450, 130, 4): dict(ch=7, cpr=19, last=4, nc=4, run_inside=True),
    (4100, 130, 4): dict(ch=64, cpr=3, last=2, nc=4, run_inside=True),
    (8200, 64, 2): dict(ch=64, cpr=1, last=64, nc=4, run_inside=True),
    (3, 40, 514): dict(ch=4, nc=8),
    (3, 9, 1024): dict(ch=4, cpr=3, last=1, nc=8),
    (3, 9, 1023): dict(ch=4, nc=8, odd=True),
    (37, 131, 64): dict(ch=4, cpr=33, last=3, nc=4, run_inside=True),
    (3, 11, 8): dict(ch=4, cpr=3, last=3, sorted_last=1),
    (5, 9, 2): dict(ch=4, cpr=3, last=1), (5, 9, 33): dict(ch=4, last=1, odd=True), (5, 9, 66): dict(ch=4, last=1),
    (5, 9, 130): dict(ch=4, last=1),
}


@pytest.mark.parametrize("case", R.NEG_CASES, ids=R.case_id)
def test_neg_cases_reach_their_branches(case):
    for slot in (0, 2):
        got = R.branches(R.make_case(case, slot))
        for name, value in NEG_BRANCHES[(case["n"], case["K"], case["d"])].items():
            assert got[name] == value, (R.case_id(case), slot, name, got)
        if got["run_inside"]:
            assert got["max_run"] > R.SORT_CH


def test_every_branch_has_a_case():
    """chunk lengths 4, one in 5..63 and 64 (ragged and full last chunks), one chunk and many per positive; NC = 4 and 8,
    the largest d, an odd d under NC = 8, d above 1024 unsupported; a last sorted chunk of one; runs longer than a sorted
    chunk inside chunks; rel_scratch for RotatE (and NULL: every RotatE case runs both in test_gpu_neg_bwd.py); pitched
    and pre-loaded tables, l_norm 2 and 3 for both distance scorers at d = 2, 33 / 66, 130; the spo chunk lengths 1, 3,
    32 with runs across chunk borders, a run of one and a ragged last chunk; n = 5 for the per-row kernel."""
    nb = [(c, R.branches(R.make_case(c, 0))) for c in R.NEG_CASES]
    chs = {b["ch"] for _, b in nb}
    assert 4 in chs and 64 in chs and any(4 < x < 64 for x in chs)
    assert any(b["ch"] == 64 and b["last"] == 64 and b["cpr"] == 1 for _, b in nb)
    assert any(b["ch"] == 64 and b["last"] < 64 and b["cpr"] > 1 for _, b in nb)
    assert {b["nc"] for _, b in nb} == {4, 8}
    assert any(c["d"] == 1024 for c, _ in nb) and any(b["nc"] == 8 and b["odd"] for _, b in nb)
    assert any(b["nc"] == 8 and c["d"] == 514 for c, b in nb)
    assert R.sorted_nc(R.NEG_UNSUPPORTED["d"]) is None and R.sorted_nc(R.ACC_UNSUPPORTED["d"]) is None
    assert any(b["sorted_last"] == 1 and c["n"] * c["K"] == 33 for c, b in nb)
    assert any(b["run_inside"] and c["E"] == 23 for c, b in nb)
    assert any(c["name"] == "rotate" and b["nc"] == 8 for c, b in nb) and any(c["name"] == "rotate" and b["nc"] == 4 for c, b in nb)
    assert sum(bool(c.get("pitched")) for c in R.NEG_CASES) >= 1 and sum(bool(c.get("pitched")) for c in R.ACC_CASES) >= 1
    assert any(c.get("pitched") and c["l_norm"] != 1.0 for c in R.NEG_CASES)  # a `scores` slice
    for name, dmid in (("transe", 33), ("rotate", 66)):
        for lp in (2.0, 3.0):
            assert {c["d"] for c in R.NEG_CASES if c["name"] == name and c["l_norm"] == lp} >= {2, dmid, 130}
    ab = [(c, R.branches(R.make_case(c))) for c in R.ACC_CASES]
    assert {b["ch"] for _, b in ab} == {1, 3, 32}
    for ch in (3, 32):
        assert any(b["ch"] == ch and b["first_run_s"] == 1 and b["run_s"] > ch and b["run_s"] % ch and b["run_p"] % ch
                   and 0 < b["last"] < ch for _, b in ab)
    assert any(c["d"] == 1024 for c, _ in ab)
    sb = [(c, R.branches(R.make_case(c))) for c in R.SPO_CASES]
    assert {c["d"] for c, _ in sb} == {1, 2, 33, 66, 130, 1024} and {c["n"] for c, _ in sb} == {1, 4, 5}
    assert any(b["second_group"] for _, b in sb)
    assert {c["l_norm"] for c, _ in sb} == {1.0, 2.0, 3.0}
