"""kge_score_pairs_bwd on bf16 ComplEx / DistMult tables (bwdg_run16, bwd_gemm.hip) restated in numpy for the tests
(no torch, no GPU), with an elementwise rounding bound.  The float32 twin is tests/_pairs_bwd_ref.py, whose closed
forms (`_dot`), index masks (`_masks`), operand gather with its planted defects (`_operands`) and host rules
(`gemm_split`, `gemm_vec`) are reused here.

What the entry does, stage by stage, and what of it is restated EXACTLY (bit for bit, pure functions of the inputs):

  bwdg_cast_kernel        G16 = RNE_bf16(gout), row pitch mp = m rounded up to 8, pad columns [m, mp) zero
  bwdg_build_q16_kernel   Q16 = RNE_bf16(fl32(q)); q = a r (ComplEx: complex product, po: conj(r) a).  A product of two
                          bf16 values is exact in float32, so fl32(q) is ONE correctly rounded float32 addition or
                          subtraction of two exact products (DistMult: the exact product) -- the library is built with
                          -ffp-contract=off, and a fused multiply-add would give the same bits anyway
  bwdg_gather16_kernel    listed target rows copied (exact)

`bf16_rne` restates v_cvt_pk_bf16_f32 (bf16_pack, common.hpp) for finite values; `q16` evaluates the kernel's
expressions in numpy float32 in the kernel's operation order.  What remains is float32 accumulation:

  dQ = G16 T              [n, d], reduction over the m targets        gemm16_kernel<false> / gemm32_kernel<u16, true>
  dT = G16^T Q16          [m, d], reduction over the n queries        gemm16_kernel<true>  / gemm32_kernel<u16, false>
  bwdg_chain16_kernel     g_a, g_p from dQ and the bf16-valued rows: two products and a sum (DistMult: one product)

`pairs_bwd16(...)` -> (g_a, g_p, g_tgt) in float64 from exactly these operands; `round_q=False` uses the unrounded q in
dT (what float64 autograd on the bf16-valued tables gives).

`pairs_bwd16_bound(...)` -> elementwise (C_ACC K + C) u A, u = 2^-24:

  A      the companion value of _pairs_bwd_ref: the same formulas on magnitudes, every subtraction an addition; for dT
         it is built on |Q16|
  K      m for g_a / g_p, n for g_tgt.  Every term of either sum is a product of two bf16 values: exact.  The split-K
         sum (bwdg_reduce_kernel) and the exchange of halves between the two K groups of gemm16_kernel are float32
         additions of the same sum: counted in K
  C      roundings behind the sum: bwdg_chain16_kernel computes dq r +- dq' r' (product 1 + sum 1 = 2) for ComplEx and
         dq r (1) for DistMult; 0 for g_tgt -- Q16 is an exact operand here, not a rounded float32 quantity
  C_ACC  = 2.  (K - 1) u bounds a float32 sum of K terms in any order only if every addition rounds to nearest.  How
         v_mfma_f32_32x32x16_bf16 rounds the additions inside one instruction (16 products and the accumulator) is
         not documented; two units per accumulated term cover additions that truncate.  THIS IS AN ASSUMPTION ABOUT
         THE MATRIX CORE, NOT A MEASUREMENT: tests/test_gpu_pairs_bwd16.py prints the largest err / bound of every
         case (profiles/pairs_bwd16_bound.txt), and a ratio above 1 there is a finding about the kernel or about
         this constant, to be told apart with the KGE_BWD_GEMM_LIB switch (the same products on gemm32_kernel) --
         never a reason to raise C_ACC to what the kernel under test produced.

The host rules are restated too (`gemm16_split`, `takes_gemm16`, `branches16`), so that the CPU file can assert which
kernel and which split every case reaches and the "last split part dropped" defect knows its indices.  The fixed case
list of tests/test_gpu_pairs_bwd16.py is built here (`CASES16`, `make_case16`): tests/test_pairs_bwd16_ref_cpu.py checks
the very inputs the GPU file runs.
"""
import numpy as np

import _pairs_bwd_ref as R

U = R.U
C_ACC = 2
C_CHAIN16 = {"complex": 2, "distmult": 1}
C_TGT16 = 0


# ---- the two operand roundings ---------------------------------------------------------------------------------------
def _bits(x32):
    return np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)


def bf16_rne(x32):
    """float32 -> the nearest bf16 value (ties to even), as a float32 array: v_cvt_pk_bf16_f32 on finite values"""
    u = _bits(x32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x32))


def bf16_trunc(x32):
    """planted defect: the low 16 bits cut off (round toward zero)"""
    return (_bits(x32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(x32))


def bf16_half_up(x32):
    """planted defect: round to nearest, ties AWAY from zero instead of to even"""
    u = _bits(x32).astype(np.uint64)
    return ((u + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(np.shape(x32))


def is_bf16_tie(x32):
    """exactly half way between two neighbouring bf16 values"""
    return (_bits(x32) & np.uint32(0xFFFF)) == np.uint32(0x8000)


def q32(name, direction, A16, R16):
    """fl32(q): the expressions of bwdg_build_q16_kernel in numpy float32, in the kernel's operation order"""
    A, Rr = np.asarray(A16, dtype=np.float32), np.asarray(R16, dtype=np.float32)
    if name == "distmult":
        return A * Rr
    h = A.shape[1] // 2
    a0, a1, r0, r1 = A[:, :h], A[:, h:], Rr[:, :h], Rr[:, h:]
    if direction == "sp":
        return np.hstack([a0 * r0 - a1 * r1, a1 * r0 + a0 * r1])
    return np.hstack([r0 * a0 + r1 * a1, r0 * a1 - r1 * a0])


def q16(name, direction, A16, R16):
    """Q16 of bwdg_build_q16_kernel as bf16-valued float32"""
    return bf16_rne(q32(name, direction, A16, R16))


# ---- the gradients and their bound -----------------------------------------------------------------------------------
def _gout16(gout, defect):
    g = np.asarray(gout, dtype=np.float32)
    if defect.get("gout_trunc"):
        G = bf16_trunc(g)
    elif defect.get("gout_half_up"):
        G = bf16_half_up(g)
    else:
        G = bf16_rne(g)
    if defect.get("cast_tail"):  # the last column lost by the cast
        G = G.copy()
        G[:, -1] = 0.0
    return G


def pairs_bwd16(name, direction, ent16, rel16, a, p, targets, gout, defect=None, round_q=True, dtype=np.float64):
    """-> (g_a, g_p, g_tgt) in float64 (module docstring).  `defect`: a planted defect, those of _pairs_bwd_ref and
         gout_trunc / gout_half_up   gout truncated / rounded half away from zero instead of RNE
         q_unrounded / q_trunc       dT from fl32(q) itself / from its truncation
         cast_tail                   the last column of gout dropped by the cast
         pad_one                     the first pad column of G16 holds 1.0: gemm16_kernel<false> multiplies it with the
                                     row its clamp reads there, the last target row
    dtype=np.float32: the same operands with every product and sum in float32, in numpy's order."""
    defect = defect or {}
    A, Rr, T = R._operands(name, ent16, rel16, a, p, targets, defect, dtype)
    G = _gout16(gout, defect).astype(dtype)
    Gm, Gn = R._masks(G, defect)
    if defect.get("pad_one"):
        Gm, T = np.hstack([Gm, np.ones((Gm.shape[0], 1), dtype)]), np.vstack([T, T[-1:]])
    ga, gp, dT = R._dot(name, direction, A, Rr, T, Gm, Gn, -1.0, bool(defect.get("flip_cross")))
    if round_q and not defect.get("q_unrounded"):
        qf = q32(name, direction, A, Rr)
        Q = bf16_trunc(qf) if defect.get("q_trunc") else bf16_rne(qf)
        dT = Gn.T @ Q.astype(dtype)
    return ga, gp, dT


def pairs_bwd16_bound(name, direction, ent16, rel16, a, p, targets, gout):
    """-> (b_a, b_p, b_tgt): |float32-accumulated result - pairs_bwd16| <= bound elementwise (module docstring)"""
    A, Rr, T = R._operands(name, ent16, rel16, a, p, targets, {})
    G = np.abs(bf16_rne(gout)).astype(np.float64)
    ca, cp, _ = R._dot(name, direction, np.abs(A), np.abs(Rr), np.abs(T), G, G, 1.0)
    ct = G.T @ np.abs(q16(name, direction, A, Rr)).astype(np.float64)
    n, m = G.shape
    cc = C_CHAIN16[name]
    return (C_ACC * m + cc) * U * ca, (C_ACC * m + cc) * U * cp, (C_ACC * n + C_TGT16) * U * ct


# ---- the host rules ----------------------------------------------------------------------------------------------------
G16_BM, G16_BN, G16_BK = 128, 256, 64


def gemm16_split(rows, m, d, scratch_bytes):
    """run_gemm16_dq (bwd_gemm16.hip): (splits, K steps of each split).  Split s takes the 64-wide K steps
    [ksteps s / splits, ksteps (s + 1) / splits) (gemm16_kernel: st_lo, st_hi)."""
    per = -(-rows // G16_BM) * (d // G16_BN)
    ksteps = -(-m // G16_BK)
    splits = min(256 // per, scratch_bytes // (rows * d * 4) if scratch_bytes else 0, ksteps)
    if splits < 2:
        splits = 1
    return splits, tuple(ksteps * (s + 1) // splits - ksteps * s // splits for s in range(splits))


def takes_gemm16(d, ldt, table_base_aligned16=True, switch=None):
    """(dQ on gemm16_kernel, dT on gemm16_kernel) as run_gemm16_dq / run_gemm16_dt decide; `switch`: the value of
    BWD_GEMM_LIB (bwd_gemm16_enabled()).  G16 and Q16 sit in the 256-byte aligned workspace on pitches mp and d, both
    multiples of 8 whenever d % 256 == 0; only dQ reads the table (pitch ldt)."""
    ok = switch != 1 and d % G16_BN == 0
    return bool(ok and ldt % 8 == 0 and table_base_aligned16), bool(ok)


def branches16(case, switch=None):
    """What one case runs through, from the host rules: the kernel of either product, the split of dQ (parts, and for
    gemm32_kernel kc), `gather` (bwdg_gather16_kernel, rows parked in g_tgt), `cast_tail` (odd m: `j + 1 < m` false in
    the last thread of a row of bwdg_cast_kernel), `pad` (columns [m, mp)), and for gemm32_kernel<unsigned short> its
    vec / inner of run_gemm32's in16 rule."""
    n, d = case["n"], case["d"]
    listed = case.get("listed")
    m = listed if listed else case["E"]
    mp = (m + 7) // 8 * 8
    ldt = d if listed else case.get("ent_ld") or d
    scratch = 0 if listed else m * d  # floats: g_tgt, unless listed rows are parked there
    dq16, dt16 = takes_gemm16(d, ldt, True, switch)
    out = dict(gather=bool(listed), cast_tail=bool(m % 2), pad=mp - m, mp=mp)
    if dq16:
        parts, steps = gemm16_split(n, m, d, scratch * 4)
        out["dq"] = dict(kernel="gemm16", parts=parts, steps=steps, ksteps=sum(steps), tail=m % G16_BK,
                         mtiles=-(-n // G16_BM), ntiles=d // G16_BN)
    else:
        parts, kc = R.gemm_split(n, d, m, scratch)
        vec = R.gemm_vec(mp, ldt, 2, 8)
        out["dq"] = dict(kernel="gemm32", parts=parts, kc=kc, vec=vec, BM=256 if n > 128 else 128,
                         inner=bool(vec and n >= (256 if n > 128 else 128) and d >= 128))
    if dt16:
        out["dt"] = dict(kernel="gemm16", ksteps=-(-n // G16_BK), tail=n % G16_BK, mtiles=-(-m // G16_BM),
                         ntiles=d // G16_BN, last_rows=m - (-(-m // G16_BM) - 1) * G16_BM)
    else:
        vec = R.gemm_vec(mp, d, 2, 8)
        BM = 256 if m > 128 else 128
        out["dt"] = dict(kernel="gemm32", parts=1, vec=vec, BM=BM, inner=bool(vec and m >= BM and d >= 128))
    return out


def last_part16(case):
    """the indices of the last part of dQ's m-reduction, or None where it is not split"""
    b = branches16(case)["dq"]
    m = case.get("listed") or case["E"]
    if b["parts"] < 2:
        return None
    lo = (sum(b["steps"][:-1]) * G16_BK) if b["kernel"] == "gemm16" else (b["parts"] - 1) * b["kc"]
    return np.arange(lo, m)


# ---- the fixed cases ---------------------------------------------------------------------------------------------------
def _case(name, n, E, d, **kw):
    return dict(name=name, l_norm=1.0, n=n, E=E, d=d, **kw)


# (the branch each shape reaches: BRANCHES16 of tests/test_pairs_bwd16_ref_cpu.py; DESIGN.md, "Mixed-precision pair
# backward against float64")
CASES16 = [
    _case("complex", 1, 1, 256),
    _case("distmult", 1, 1, 256),
    _case("complex", 37, 150, 256),
    _case("distmult", 37, 150, 256),
    _case("complex", 130, 200, 256),
    _case("distmult", 129, 257, 512),
    _case("complex", 64, 64, 256),
    _case("distmult", 65, 64, 256),
    _case("complex", 5, 2177, 256),
    _case("complex", 16, 1000, 256, listed=300),
    _case("distmult", 37, 150, 256, ent_ld=264),
    _case("complex", 37, 150, 256, ent_ld=260),
    _case("complex", 37, 150, 256, gout_ld=152),
    _case("complex", 37, 150, 256, triples32=True),
    _case("complex", 37, 150, 40),
    _case("distmult", 70, 150, 130),
    _case("complex", 128, 256, 128),
]

case_id = R.case_id
N_TIES = 16  # planted in gout where n m >= 64


def make_case16(c, direction, seed=None):
    """The inputs of one case and direction: the dict of _pairs_bwd_ref.make_case (ent, rel float32 arrays of
    bf16-VALUED numbers) plus
      tie_pos   flat positions in gout [n, m] of the planted bf16 rounding ties ((k + 1/2) 2^-8, k even and odd, both
                signs: RNE, round-half-up, round-half-down and truncation all differ on them), empty where n m < 64
      q_ties    how many elements of fl32(q) are exact bf16 ties
    gout: float32 magnitudes in [0.5, 1], none bf16-representable, none a tie but the planted ones; where no ties
    are planted (n m < 64) every element lies in the upper half of its bf16 interval, so that truncation differs from
    RNE in each."""
    name, n, E, d = c["name"], c["n"], c["E"], c["d"]
    if seed is None:
        seed = 1000 * CASES16.index(c) + (0 if direction == "sp" else 1) + 160000
    rng = np.random.default_rng(seed)
    nrel = 7
    listed = c.get("listed")
    m = listed if listed else E
    p = rng.integers(0, nrel, n)
    a = rng.integers(0, E, n)
    targets = None
    if listed:  # with duplicates: every third entry repeats its predecessor's row
        targets = rng.integers(0, E, m)
        targets[2::3] = targets[1::3][: len(targets[2::3])]
    ent, rel = bf16_rne(R._mag(rng, (E, d))), bf16_rne(R._mag(rng, (nrel, d)))
    gout = R._mag(rng, (n, m))
    u = gout.view(np.uint32)
    low = u & np.uint32(0xFFFF)
    u[(low == 0) | (low == 0x8000)] += np.uint32(1)
    tie_pos = np.zeros(0, np.int64)
    if n * m >= 64:
        tie_pos = np.unique(np.linspace(0, n * m - 1, N_TIES).astype(np.int64))
        i = np.arange(tie_pos.size)
        k = 130 + 7 * i  # alternating parity, below 256
        sign = np.where((i // 2) % 2 == 0, 1.0, -1.0)
        gout.reshape(-1)[tie_pos] = (sign * (k + 0.5) * 2.0 ** -8).astype(np.float32)
    else:
        u |= np.uint32(0x8000)
        u[(u & np.uint32(0xFFFF)) == 0x8000] += np.uint32(1)
    out = dict(c)
    out.update(direction=direction, ent=ent, rel=rel, a=a.astype(np.int64), p=p.astype(np.int64),
               targets=None if targets is None else targets.astype(np.int64), gout=gout, m=m, listed=bool(listed),
               tie_pos=tie_pos, q_ties=int(is_bf16_tie(q32(name, direction, ent[a], rel[p])).sum()))
    return out


def ref_args16(k):
    return (k["name"], k["direction"], k["ent"], k["rel"], k["a"], k["p"], k["targets"], k["gout"])
