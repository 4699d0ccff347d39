"""tests/_pairs_bwd_ref.py checked on the CPU: the float64 closed forms against float64 torch autograd through
oracle/torch_port.py, the rounding bound against planted defects on the very inputs of tests/test_gpu_pairs_bwd.py
(a defect must exceed the bound 8 times over: the bound is sharp enough to see it), and the inputs themselves."""
import numpy as np
import pytest
import torch

import torch_port as tp
import _pairs_bwd_ref as R

SHARP = 8.0
LONG_K = 700  # above this reduction length one dropped index may stay below 8 x bound; a block / a part must not

SMALL = [(name, lp, listed)
         for name in ("complex", "distmult", "transe", "rotate")
         for lp in ((1.0, 2.0, 3.0) if name in ("transe", "rotate") else (1.0,))
         for listed in (None, 7)]


@pytest.mark.parametrize("name,lp,listed", SMALL, ids=[f"{n}-L{l:g}-{'listed' if t else 'all'}" for n, l, t in SMALL])
@pytest.mark.parametrize("direction", ["sp", "po"])
def test_reference_matches_float64_autograd(name, lp, listed, direction):
    """pairs_bwd, its per-row outputs scattered into tables, == autograd of torch_port.score_sp / score_po in float64
    (1e-12 of the largest gradient).  The TransE inputs carry exact ties: sign(0) = 0, as cdist's backward has it."""
    c = dict(name=name, l_norm=lp, n=5, E=9, d=6)
    if listed:
        c["listed"] = listed
    k = R.make_case(c, direction, seed=17)
    if name == "transe":
        assert R.transe_ties(direction, k["ent"], k["rel"], k["a"], k["p"], k["targets"]) > 0
    g_a, g_p, g_t = R.pairs_bwd(*R.ref_args(k))
    ent = torch.tensor(k["ent"], dtype=torch.float64, requires_grad=True)
    rel = torch.tensor(k["rel"], dtype=torch.float64, requires_grad=True)
    a, p = torch.tensor(k["a"]), torch.tensor(k["p"])
    tg = None if k["targets"] is None else torch.tensor(k["targets"])
    sc = tp.score_sp(name, ent, rel, a, p, tg, lp) if direction == "sp" else tp.score_po(name, ent, rel, p, a, tg, lp)
    (sc * torch.tensor(k["gout"], dtype=torch.float64)).sum().backward()
    ge = np.zeros_like(ent.grad.numpy())
    np.add.at(ge, k["a"], g_a)
    np.add.at(ge, np.arange(k["E"]) if k["targets"] is None else k["targets"], g_t)
    gr = np.zeros_like(rel.grad.numpy())
    np.add.at(gr, k["p"], g_p)
    for got, want in ((ge, ent.grad.numpy()), (gr, rel.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _defects(k):
    """(label, defect, outputs it must show in, required) for one case.  Where a reduction is shorter than 32 (n or m in
    1, 3, 5, 15, 16, 17) the aligned block covers all of it: the block defect then drops the whole sum and adds
    nothing to the single-index one."""
    n, m = k["n"], k["m"]
    blk = lambda K: np.arange(max(0, (K // 32 - 1) * 32), max(0, (K // 32 - 1) * 32) + min(32, K))
    out = [("last m index", dict(drop_m=[m - 1]), (0, 1), m <= LONG_K),
           ("last n index", dict(drop_n=[n - 1]), (2,), n <= LONG_K),
           ("32 m indices", dict(drop_m=blk(m)), (0, 1), True),
           ("32 n indices", dict(drop_n=blk(n)), (2,), True),
           ("last coordinate zero", dict(zero_last=True), (0, 1, 2), True)]
    part = R.last_part(k)
    if part is not None:
        out.append(("last part of the split", dict(drop_m=part), (0, 1), True))
    if k["name"] == "complex":
        out.append(("cross term sign", dict(flip_cross=True), (0,), True))
    if n > 1 and (k["p"] != np.roll(k["p"], -1)).any():
        out.append(("next row's relation", dict(rel_next=True), (0, 1, 2), True))
    if k["name"] == "transe" and k["l_norm"] == 1.0 and (k["E"], k["d"]) != (1, 1):
        # the spo path's epsilon (F.pairwise_distance) taken over into the pair path, which has none (torch.cdist):
        # every exact tie then weighs sign(1e-6) = 1 instead of 0
        out.append(("1e-6 at the ties", dict(eps=1e-6), (0, 1, 2), True))
    return out


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_bound_is_sharp_and_inputs_well_posed(case):
    for direction in ("sp", "po"):
        k = R.make_case(case, direction)
        args = R.ref_args(k)
        if case["name"] == "transe":
            # the dyadic grid (planted ties reach 4): differences exact in float32 and float64 alike
            for x in (k["ent"], k["rel"]):
                assert (np.abs(x) <= 4.0).all() and (x * 64 == np.round(x * 64)).all()
            assert R.transe_ties(direction, *args[3:8]) > 0 or (case["E"], case["d"]) == (1, 1)
        if case["name"] == "rotate":
            assert R.rotate_min_modulus(direction, *args[3:]) >= 2.0 ** -6
        want = R.pairs_bwd(*args)
        bound = R.pairs_bwd_bound(*args)
        for w, b in zip(want, bound):
            assert np.isfinite(w).all() and np.isfinite(b).all() and (b >= 0).all()
        # one more float32 evaluation (numpy's order): inside the bound
        for g, w, b in zip(R.pairs_bwd(*args, dtype=np.float32), want, bound):
            assert (np.abs(g.astype(np.float64) - w) <= b).all(), (R.case_id(case), direction)
        for label, defect, outs, required in _defects(k):
            bad = R.pairs_bwd(*args, defect=defect)
            ratio = max(float((np.abs(bad[o] - want[o]) / np.maximum(bound[o], 1e-300)).max()) for o in outs)
            if required:
                assert ratio >= SHARP, (R.case_id(case), direction, label, ratio)


# The branch list of DESIGN.md section 21, as the restated host rules (gemm_vec, gemm_split) give it: per case the facts
# about the dQ product (M = n, K = m) and the dT product (M = m, K = n) the shape was chosen for.
DOT_BRANCHES = {
    "complex-n1-E1-d2": (dict(vec=0, nchunk=1, parts=1), dict(vec=0, nchunk=1)),
    "distmult-n1-E1-d1": (dict(vec=0, nchunk=1, parts=1), dict(vec=0, nchunk=1)),
    "complex-n37-E150-d40": (dict(vec=0, BM=128, parts=2, kc=96), dict(vec=0, BM=256, nchunk=2)),
    "distmult-n37-E150-d40": (dict(vec=0, BM=128, parts=2, kc=96), dict(vec=0, BM=256, nchunk=2)),
    "complex-n128-E256-d128": (dict(vec=1, inner=True, BM=128, parts=2, kc=128), dict(vec=1, inner=True, BM=256)),
    "complex-n129-E257-d132": (dict(vec=0, BM=256, parts=1), dict(vec=0, BM=256)),
    "complex-n129-E257-d132-gout_ld260": (dict(vec=1, BM=256, parts=1, a_tail=True, b_tail=False),
                                          dict(vec=1, BM=256, inner=True, a_tail=True)),
    "complex-n70-E150-d130-ent_ld132-gout_ld152": (dict(vec=1, parts=2, kc=96, a_tail=True, b_tail=True), dict(vec=0)),
    "distmult-n70-E150-d130-ent_ld132-gout_ld152": (dict(vec=1, parts=2, kc=96, a_tail=True, b_tail=True), dict(vec=0)),
    "distmult-n3-E200-d33": (dict(vec=0, parts=1, nchunk=7), dict(vec=0, nchunk=1)),
    "complex-n130-E200-d40": (dict(vec=1, BM=256, parts=1, nchunk=7), dict(vec=1, BM=256)),
    "complex-n5-E2177-d8": (dict(vec=0, parts=23, kc=96), dict(vec=0, nchunk=1)),
    "complex-n33-E300-d24": (dict(vec=1, parts=4, kc=96), dict(vec=1, BM=256, nchunk=2)),
    "distmult-n64-E300-d24": (dict(vec=1, parts=4, kc=96), dict(vec=1, BM=256, nchunk=2)),
    "complex-n65-E300-d24": (dict(vec=1, parts=4, kc=96), dict(vec=1, BM=256, nchunk=3)),
    "complex-n16-E1000-d40-listed300": (dict(vec=1, parts=1, nchunk=10), dict(vec=1, BM=256, nchunk=1)),
    "complex-n37-E150-d40-triples32": (dict(vec=0, parts=2, kc=96), dict(vec=0, nchunk=2)),
}


@pytest.mark.parametrize("case", R.DOT_CASES, ids=R.case_id)
def test_dot_cases_reach_their_branches(case):
    got = R.dot_branches(case)
    for key, want in zip(("dq", "dt"), DOT_BRANCHES[R.case_id(case)]):
        for name, value in want.items():
            assert got[key][name] == value, (R.case_id(case), key, name, got[key])


def test_every_gemm_branch_has_a_case():
    """vec = 0 and 1, both tile heights, `inner` loads, g32_load4 tails with vec = 1 on B (an N tail) and on A of either
    layout, split and unsplit long K: each reached by one case at least, in the product named."""
    b = [R.dot_branches(c) for c in R.DOT_CASES]
    for key in ("dq", "dt"):
        assert {x[key]["vec"] for x in b} == {0, 1} and any(x[key]["inner"] for x in b)
        assert any(x[key]["a_tail"] for x in b)
    assert {x["dq"]["BM"] for x in b} == {128, 256} and any(x["dt"]["BM"] == 256 for x in b)
    assert any(x["dq"]["b_tail"] for x in b)  # (dT's B is the query matrix on pitch d: vec = 1 there means d % 4 == 0)
    assert any(x["dq"]["parts"] > 1 for x in b) and any(x["dq"]["parts"] == 1 and x["dq"]["nchunk"] > 4 for x in b)
    assert {x["dt"]["nchunk"] for x in b} >= {1, 2, 3}


def test_split_rules_name_the_branches():
    """The host split rules restated for the part defect give the parts the case list was chosen for."""
    assert R.gemm_split(37, 40, 150, 150 * 40) == (2, 96)          # two parts, the second ragged (54)
    assert R.gemm_split(128, 128, 256, 256 * 128) == (2, 128)      # two aligned parts
    assert R.gemm_split(3, 33, 200, 200 * 33) == (1, 200)          # (M N) % 4 != 0
    assert R.gemm_split(130, 40, 200, 200 * 40) == (1, 200)        # scratch for one partial only
    assert R.gemm_split(5, 8, 2177, 2177 * 8) == (23, 96)          # many parts, the last 65 long
    assert R.gemm_split(16, 40, 300, 0) == (1, 300)                # listed targets: no scratch
    assert R.pairs_split(130, 150, 66) == (10, 16)
    assert R.pairs_split(65, 17, 64) == (2, 16)
    assert R.pairs_split(63, 16, 2) == (1, 16)
    assert R.pairs_split(1, 1037, 130) == (22, 48)
    assert R.pairs_split(1, 150, 2) == (10, 16)
