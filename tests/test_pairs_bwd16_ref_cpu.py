"""tests/_pairs_bwd16_ref.py checked on the CPU: the float64 reference of the mixed-precision pair backward against
float64 torch autograd through oracle/torch_port.py, the two restated bf16 roundings, the rounding bound against a
float32 evaluation and against planted defects on the very inputs of tests/test_gpu_pairs_bwd16.py (a defect must
exceed the bound 8 times over: the bound is sharp enough to see it), and the branch every case reaches."""
import numpy as np
import pytest
import torch

import oracle
import torch_port as tp
import _pairs_bwd_ref as R
import _pairs_bwd16_ref as R16

SHARP = 8.0
LONG_K = 700   # the carried-over defects: required where the affected reduction has 2 .. 700 terms
ROUND_K = 64   # the rounding-stage defects: required where it has at most 64 terms (DESIGN.md has the ratios beyond)


def _exact_q(name, direction, A, Rr):
    """q in float64 through _dot's own closed form (dT = I^T q): sums of two 16-bit products, exact in float64"""
    n = A.shape[0]
    return R._dot(name, direction, A.astype(np.float64), Rr.astype(np.float64), np.zeros(A.shape), np.eye(n), np.eye(n),
                  -1.0)[2]


# ---- reference against autograd ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["complex", "distmult"])
@pytest.mark.parametrize("listed", [None, 7], ids=["all", "listed"])
@pytest.mark.parametrize("direction", ["sp", "po"])
def test_reference_matches_float64_autograd(name, listed, direction):
    """round_q=False: pairs_bwd16, its per-row outputs scattered into tables, == float64 autograd of torch_port.score_sp /
    score_po on the bf16-valued tables with bf16_rne(gout) as upstream gradient (1e-12 of the largest gradient).
    round_q=True: g_a and g_p are the same bits; g_tgt moves by at most 2^-9 (|G16|^T |q|) elementwise.  (Rounding q to
    the 8 significant bits of bf16 moves ONE term by up to 2^-8 of itself, 2^-10 of itself in the mean: 2^-9 of the sum of
    magnitudes is no guarantee for a sum of a few terms -- with n = 5 these inputs reach 1.4 times it -- but holds with
    a wide margin once the sum has some tens of terms of mixed sign, hence n = 33 here.)"""
    c = dict(name=name, l_norm=1.0, n=33, E=9, d=6)
    if listed:
        c["listed"] = listed
    k = R16.make_case16(c, direction, seed=17)
    if listed:
        assert len(set(k["targets"].tolist())) < len(k["targets"])
    args = R16.ref_args16(k)
    g_a, g_p, g_t = R16.pairs_bwd16(*args, round_q=False)
    ent = torch.tensor(k["ent"], dtype=torch.float64, requires_grad=True)
    rel = torch.tensor(k["rel"], dtype=torch.float64, requires_grad=True)
    a, p = torch.tensor(k["a"]), torch.tensor(k["p"])
    tg = None if k["targets"] is None else torch.tensor(k["targets"])
    sc = tp.score_sp(name, ent, rel, a, p, tg) if direction == "sp" else tp.score_po(name, ent, rel, p, a, tg)
    G16 = R16.bf16_rne(k["gout"]).astype(np.float64)
    (sc * torch.tensor(G16)).sum().backward()
    ge = np.zeros_like(ent.grad.numpy())
    np.add.at(ge, k["a"], g_a)
    np.add.at(ge, np.arange(k["E"]) if k["targets"] is None else k["targets"], g_t)
    gr = np.zeros_like(rel.grad.numpy())
    np.add.at(gr, k["p"], g_p)
    for got, want in ((ge, ent.grad.numpy()), (gr, rel.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    r_a, r_p, r_t = R16.pairs_bwd16(*args, round_q=True)
    assert np.array_equal(r_a, g_a) and np.array_equal(r_p, g_p)
    lim = 2.0 ** -9 * (np.abs(G16).T @ np.abs(_exact_q(name, direction, k["ent"][k["a"]], k["rel"][k["p"]])))
    assert (np.abs(r_t - g_t) <= lim).all() and np.abs(r_t - g_t).max() > 0


# ---- the rounding restatements -----------------------------------------------------------------------------------------
def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_bf16_rne_on_ties_neighbours_zero_and_the_largest_finite():
    k = R16.make_case16(R16.CASES16[2], "sp")
    ties = k["gout"].reshape(-1)[k["tie_pos"]]
    assert ties.size == R16.N_TIES and R16.is_bf16_tie(ties).all()
    assert not R16.is_bf16_tie(np.delete(k["gout"].reshape(-1), k["tie_pos"])).any()
    u = ties.view(np.uint32)
    lo, hi = _f(u & 0xFFFF0000), _f((u & 0xFFFF0000) + 0x10000)  # the two bf16 neighbours (by magnitude)
    even_lo = ((u >> 16) & 1) == 0
    assert even_lo.any() and (~even_lo).any() and (ties > 0).any() and (ties < 0).any()
    assert np.array_equal(R16.bf16_rne(ties), np.where(even_lo, lo, hi))      # ties to even
    assert np.array_equal(R16.bf16_rne(_f(u - 1)), lo)                        # one float32 ulp inside: down
    assert np.array_equal(R16.bf16_rne(_f(u + 1)), hi)                        # one float32 ulp beyond: up
    # the planted defects differ from RNE on ties: half-up where the lower neighbour is even, truncation (and
    # round-half-down) where it is odd
    assert np.array_equal(R16.bf16_half_up(ties) != R16.bf16_rne(ties), even_lo)
    assert np.array_equal(R16.bf16_trunc(ties) != R16.bf16_rne(ties), ~even_lo)
    z = R16.bf16_rne(_f([0x00000000, 0x80000000]))
    assert z.view(np.uint32).tolist() == [0x00000000, 0x80000000]             # +-0 keep their sign
    # 0x7f7f7fff: the largest float32 that rounds to a finite bf16 (0x7f7f); the tie above it goes to infinity
    assert R16.bf16_rne(_f([0x7F7F7FFF, 0xFF7F7FFF])).view(np.uint32).tolist() == [0x7F7F0000, 0xFF7F0000]
    assert np.isinf(R16.bf16_rne(_f([0x7F7F8000]))).all()
    # the same rule as the oracle's (bit patterns), on random values, ties and their neighbours
    x = np.concatenate([k["gout"].reshape(-1), ties, _f(u - 1), _f(u + 1), k["ent"].reshape(-1) * 3.1])
    assert np.array_equal(R16.bf16_rne(x).view(np.uint32) >> 16, oracle.f32_to_bf16(x).astype(np.uint32))
    assert np.array_equal(R16.bf16_rne(k["ent"]), k["ent"]) and np.array_equal(R16.bf16_rne(k["rel"]), k["rel"])


@pytest.mark.parametrize("case", R16.CASES16, ids=R16.case_id)
def test_q16_is_the_rounding_of_the_exact_query(case):
    """q16 == RNE to bf16 of the float64-exact q wherever fl32(q) is not within one float32 ulp of a bf16 tie (double
    rounding can only bite there); the exceptions -- elements where the two differ -- are counted: fewer than 1 % of the
    elements.  (On these inputs there is none: the operands are multiples of 2^-8 below 1, so q is a multiple of 2^-16
    below 2 and fl32(q) == q.  The elements NEAR a tie are no rarity for the same reason -- 1 in 256 where |q| is in
    [1/2, 1), 1 in 64 where cancellation leaves |q| in [1/8, 1/4): 1 to 3 % of a ComplEx query matrix.)"""
    for direction in ("sp", "po"):
        k = R16.make_case16(case, direction)
        A, Rr = k["ent"][k["a"]], k["rel"][k["p"]]
        qf = R16.q32(k["name"], direction, A, Rr)
        qx = _exact_q(k["name"], direction, A, Rr)
        assert np.array_equal(qf, qx.astype(np.float32))  # one correctly rounded float32 operation
        low = qf.view(np.uint32) & 0xFFFF
        near = (low >= 0x7FFF) & (low <= 0x8001)
        # RNE of the exact value straight to bf16: the neighbour nearer to qx, the even one on an exact tie
        lo = R16.bf16_trunc(qf).astype(np.float64)
        hi = (R16._bits(R16.bf16_trunc(qf)) + np.uint32(0x10000)).view(np.float32).astype(np.float64)
        dlo, dhi = np.abs(qx - lo), np.abs(hi - qx)
        even_lo = ((R16._bits(qf) >> 16) & 1) == 0
        direct = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(even_lo, lo, hi)))
        got = R16.q16(k["name"], direction, A, Rr).astype(np.float64)
        assert np.array_equal(got[~near], direct[~near])
        assert (got != direct).mean() < 0.01, (R16.case_id(case), direction, float((got != direct).mean()))
        if k["name"] == "distmult":  # the product is exact in float32: no double rounding at all
            assert np.array_equal(got, direct)


def test_query_ties_occur():
    """fl32(q) hits exact bf16 ties on its own (DistMult: a 16-bit product, about one element in 256)"""
    counts = {R16.case_id(c): min(R16.make_case16(c, d)["q_ties"] for d in ("sp", "po")) for c in R16.CASES16}
    assert sum(v > 0 for v in counts.values()) >= 2, counts


# ---- the bound: holds for a float32 evaluation, sharp against planted defects -------------------------------------------
def _in(K, lo, hi):
    return lo <= K <= hi


def defects16(k):
    """(label, defect, {output: reduction length}, (lo, hi)) for one case: required where an affected output's reduction
    length lies in [lo, hi], measured on those outputs."""
    n, m = k["n"], k["m"]
    blk = lambda K: np.arange(max(0, (K // 32 - 1) * 32), max(0, (K // 32 - 1) * 32) + min(32, K))
    Km, Kn, Kall = {0: m, 1: m}, {2: n}, {0: m, 1: m, 2: n}
    old, new = (2, LONG_K), (1, ROUND_K)
    out = [("last m index", dict(drop_m=[m - 1]), Km, old),
           ("last n index", dict(drop_n=[n - 1]), Kn, old),
           ("32 m indices", dict(drop_m=blk(m)), Km, old),
           ("32 n indices", dict(drop_n=blk(n)), Kn, old),
           ("last coordinate zero", dict(zero_last=True), Km, old)]
    part = R16.last_part16(k)
    if part is not None:
        out.append(("last part of the split", dict(drop_m=part), Km, old))
    if k["name"] == "complex":
        out.append(("cross term sign", dict(flip_cross=True), {0: m}, old))
    if n > 1 and (k["p"] != np.roll(k["p"], -1)).any():
        out.append(("next row's relation", dict(rel_next=True), Kall, old))
    out += [("gout truncated", dict(gout_trunc=True), Kall, new),
            ("Q unrounded in dT", dict(q_unrounded=True), Kn, new),
            ("Q truncated", dict(q_trunc=True), Kn, new)]
    if k["tie_pos"].size:
        out.append(("gout ties rounded half up", dict(gout_half_up=True), Kall, new))
    if m % 2:
        out.append(("odd m: last column dropped by the cast", dict(cast_tail=True), Kall, new))
    if m % 8:
        out.append(("pad column holds 1.0", dict(pad_one=True), Km, new))
    return out


def defect_ratios(case, direction):
    """[(label, required, ratio over the outputs the rule names (all affected ones if none), their reduction lengths)]"""
    k = R16.make_case16(case, direction)
    args = R16.ref_args16(k)
    want, bound = R16.pairs_bwd16(*args), R16.pairs_bwd16_bound(*args)
    rows = []
    for label, defect, Ks, (lo, hi) in defects16(k):
        bad = R16.pairs_bwd16(*args, defect=defect)
        outs = [o for o, K in Ks.items() if _in(K, lo, hi)]
        ratio = max(float((np.abs(bad[o] - want[o]) / np.maximum(bound[o], 1e-300)).max()) for o in (outs or Ks))
        rows.append((label, bool(outs), ratio, sorted({Ks[o] for o in (outs or Ks)})))
    return rows


@pytest.mark.parametrize("case", R16.CASES16, ids=R16.case_id)
def test_bound_holds_in_float32_and_is_sharp(case):
    for direction in ("sp", "po"):
        k = R16.make_case16(case, direction)
        args = R16.ref_args16(k)
        want, bound = R16.pairs_bwd16(*args), R16.pairs_bwd16_bound(*args)
        for w, b in zip(want, bound):
            assert np.isfinite(w).all() and np.isfinite(b).all() and (b > 0).all()
        # the whole pipeline in numpy float32 (numpy's summation order) on the exact G16 / Q16: inside the bound
        for g, w, b in zip(R16.pairs_bwd16(*args, dtype=np.float32), want, bound):
            assert g.dtype == np.float32 and (np.abs(g.astype(np.float64) - w) <= b).all(), (R16.case_id(case), direction)
        for label, required, ratio, Ks in defect_ratios(case, direction):
            if required:
                assert ratio >= SHARP, (R16.case_id(case), direction, label, ratio, Ks)


def test_every_new_defect_is_required_somewhere():
    seen = {}
    for c in R16.CASES16:
        for label, required, _, _ in defect_ratios(c, "sp"):
            seen[label] = seen.get(label, False) or required
    assert all(seen.values()) and len(seen) == 14, seen


# ---- the branch table --------------------------------------------------------------------------------------------------
# Per case: the kernel of dQ, the kernel of dT, the parts of dQ's split, bwdg_gather16_kernel, the cast's odd-m tail --
# and further facts of branches16 the shape was chosen for.
BRANCHES16 = {
    "complex-n1-E1-d256": dict(dq="gemm16", dt="gemm16", splits=1, gather=False, cast_tail=True, pad=7, mp=8,
                               dq_more=dict(ksteps=1, tail=1), dt_more=dict(ksteps=1, tail=1)),
    "distmult-n1-E1-d256": dict(dq="gemm16", dt="gemm16", splits=1, gather=False, cast_tail=True, pad=7, mp=8,
                                dq_more=dict(ksteps=1, tail=1), dt_more=dict(ksteps=1, tail=1)),
    "complex-n37-E150-d256": dict(dq="gemm16", dt="gemm16", splits=3, gather=False, cast_tail=False,
                                  dq_more=dict(steps=(1, 1, 1), tail=22)),
    "distmult-n37-E150-d256": dict(dq="gemm16", dt="gemm16", splits=3, gather=False, cast_tail=False,
                                   dq_more=dict(steps=(1, 1, 1), tail=22)),
    "complex-n130-E200-d256": dict(dq="gemm16", dt="gemm16", splits=1, gather=False, cast_tail=False,
                                   dq_more=dict(mtiles=2, ksteps=4), dt_more=dict(mtiles=2, ksteps=3, tail=2)),
    "distmult-n129-E257-d512": dict(dq="gemm16", dt="gemm16", splits=1, gather=False, cast_tail=True, pad=7, mp=264,
                                    dq_more=dict(mtiles=2, ntiles=2), dt_more=dict(mtiles=3, ntiles=2, last_rows=1)),
    "complex-n64-E64-d256": dict(dq="gemm16", dt="gemm16", splits=1, gather=False, cast_tail=False, pad=0,
                                 dq_more=dict(ksteps=1, tail=0), dt_more=dict(ksteps=1, tail=0)),
    "distmult-n65-E64-d256": dict(dq="gemm16", dt="gemm16", splits=1, gather=False, cast_tail=False,
                                  dt_more=dict(ksteps=2, tail=1)),
    "complex-n5-E2177-d256": dict(dq="gemm16", dt="gemm16", splits=35, gather=False, cast_tail=True,
                                  dq_more=dict(steps=(1,) * 35, tail=1)),
    "complex-n16-E1000-d256-listed300": dict(dq="gemm16", dt="gemm16", splits=1, gather=True, cast_tail=False,
                                             dq_more=dict(ksteps=5, tail=44)),
    "distmult-n37-E150-d256-ent_ld264": dict(dq="gemm16", dt="gemm16", splits=3, gather=False, cast_tail=False),
    "complex-n37-E150-d256-ent_ld260": dict(dq="gemm32", dt="gemm16", splits=2, gather=False, cast_tail=False,
                                            dq_more=dict(kc=96, vec=1)),
    "complex-n37-E150-d256-gout_ld152": dict(dq="gemm16", dt="gemm16", splits=3, gather=False, cast_tail=False),
    "complex-n37-E150-d256-triples32": dict(dq="gemm16", dt="gemm16", splits=3, gather=False, cast_tail=False),
    "complex-n37-E150-d40": dict(dq="gemm32", dt="gemm32", splits=2, gather=False, cast_tail=False,
                                 dq_more=dict(kc=96, vec=1, inner=False), dt_more=dict(vec=1, inner=False, BM=256)),
    "distmult-n70-E150-d130": dict(dq="gemm32", dt="gemm32", splits=2, gather=False, cast_tail=False,
                                   dq_more=dict(kc=96, vec=0), dt_more=dict(vec=0)),
    "complex-n128-E256-d128": dict(dq="gemm32", dt="gemm32", splits=2, gather=False, cast_tail=False,
                                   dq_more=dict(kc=128, vec=1, inner=True), dt_more=dict(vec=1, inner=True, BM=256)),
}


@pytest.mark.parametrize("case", R16.CASES16, ids=R16.case_id)
def test_cases_reach_their_branches(case):
    want, got = BRANCHES16[R16.case_id(case)], R16.branches16(case)
    assert got["dq"]["kernel"] == want["dq"] and got["dt"]["kernel"] == want["dt"]
    assert got["dq"]["parts"] == want["splits"]
    for key in ("gather", "cast_tail", "pad", "mp"):
        if key in want:
            assert got[key] == want[key], (key, got)
    for side in ("dq", "dt"):
        for name, value in want.get(side + "_more", {}).items():
            assert got[side][name] == value, (R16.case_id(case), side, name, got[side])
    # with the switch set, both products of every case go to gemm32_kernel
    off = R16.branches16(case, switch=1)
    assert off["dq"]["kernel"] == off["dt"]["kernel"] == "gemm32"


def test_every_branch_has_a_case():
    assert set(BRANCHES16) == {R16.case_id(c) for c in R16.CASES16}
    b = [R16.branches16(c) for c in R16.CASES16]
    kinds = {(x["dq"]["kernel"], x["dt"]["kernel"]) for x in b}
    assert kinds == {("gemm16", "gemm16"), ("gemm32", "gemm16"), ("gemm32", "gemm32")}
    g16 = [x for x in b if x["dq"]["kernel"] == "gemm16"]
    assert any(x["dq"]["parts"] == 1 for x in g16) and any(x["dq"]["parts"] == 3 for x in g16)
    assert any(x["dq"]["parts"] > 8 for x in g16)                         # more splits than one XCD round of block ids
    assert any(x["dq"]["parts"] == 1 and x["dq"]["ksteps"] > 3 and x["dq"]["tail"] for x in g16)  # the ring wraps
    assert any(x["dq"]["mtiles"] == 2 for x in g16) and any(x["dq"]["ntiles"] == 2 for x in g16)
    assert any(x["gather"] for x in b) and any(x["cast_tail"] and x["mp"] > 8 for x in b)
    assert any(x["pad"] == 0 for x in b) and any(x["pad"] == 7 for x in b)
    assert any(x["dt"]["kernel"] == "gemm16" and x["dt"]["last_rows"] == 1 and x["dt"]["mtiles"] == 3 for x in b)
    assert {x["dt"]["tail"] for x in b if x["dt"]["kernel"] == "gemm16"} >= {0, 1}
    g32 = [x for x in b if x["dq"]["kernel"] == "gemm32" and x["dt"]["kernel"] == "gemm32"]
    assert {x["dq"]["vec"] for x in g32} == {0, 1} and {x["dt"]["vec"] for x in g32} == {0, 1}
    assert any(x["dq"]["inner"] for x in g32) and any(x["dt"]["inner"] for x in g32)
    assert all(x["dq"]["parts"] > 1 for x in g32)


def test_host_rules_restated():
    assert R16.gemm16_split(37, 150, 256, 150 * 256 * 4) == (3, (1, 1, 1))       # fit 4, three K steps: last 22 long
    assert R16.gemm16_split(130, 200, 256, 200 * 256 * 4) == (1, (4,))           # scratch for one partial only
    assert R16.gemm16_split(5, 2177, 256, 2177 * 256 * 4) == (35, (1,) * 35)     # one K step each, the last 1 long
    assert R16.gemm16_split(16, 300, 256, 0) == (1, (5,))                        # listed targets: no scratch
    splits, steps = R16.gemm16_split(512, 14541, 512, 14541 * 512 * 4)   # the benchmark's shape: uneven K ranges
    assert splits == 28 and sum(steps) == 228 and set(steps) == {8, 9}
    assert R16.takes_gemm16(256, 256) == (True, True) and R16.takes_gemm16(256, 264) == (True, True)
    assert R16.takes_gemm16(256, 260) == (False, True)                           # ldt & 7: dQ declined, dT taken
    assert R16.takes_gemm16(256, 256, False) == (False, True)                    # table base not 16-byte aligned
    assert R16.takes_gemm16(40, 40) == (False, False) and R16.takes_gemm16(512, 512, True, 1) == (False, False)
    assert R.gemm_vec(152, 40, 2, 8) == 1 and R.gemm_vec(152, 130, 2, 8) == 0 and R.gemm_vec(152, 130) == 0
