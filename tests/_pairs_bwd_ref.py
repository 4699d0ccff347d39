"""kge_score_pairs_bwd restated in numpy float64 for the tests (no torch, no GPU), with an elementwise rounding bound.

`pairs_bwd(name, l_norm, direction, ent, rel, a, p, targets, gout)` -> (g_a [n, d], g_p [n, d_r], g_tgt [m, d]): the
gradients of sum_ij gout[i, j] * score(i, j) with respect to the gathered entity row, the gathered relation row and the
target rows -- per gathered row, as the ABI entry returns them, not scattered into tables.  The closed forms come from
the scorer definitions (kge/model/complex.py, distmult.py, transe.py, rotate.py; oracle/torch_port.py restates them):

  complex   sp: q = a r (complex product), po: q = conj(r) a;  score = <q, t>  (real and imaginary halves)
  distmult  q = a * r;  score = <q, t>
  transe    sp: q = a + r, po: q = a - r;  score = -||q - t||_p   (torch.cdist: NO epsilon is added to the difference
            on the sp_ / _po path -- F.pairwise_distance's 1e-6 belongs to the spo path only, bwd_device.hpp
            spo_pair_grads; sign(0) = 0 and a zero distance gives zero weight, cdist's backward)
  rotate    sp: q = a e^{i r}, po: q = e^{-i r} a;  score = -|| |q - t| ||_p over the complex coordinates

`pairs_bwd_bound(...)` -> (b_a, b_p, b_tgt), the elementwise bound (K + C) u A on a float32 evaluation, u = 2^-24:

  A  the COMPANION value: the same formulas with every operand replaced by its magnitude and every subtraction by an
     addition (cos and sin by 1: their error is absolute).  A quantity x is carried as (x, S_x, c_x) with the
     first-order guarantee |fl(x) - x| <= c_x u S_x and S_x >= |x|:
         inputs          S = |x|, c = 0
         x +- y          S = S_x + S_y,  c = max(c_x, c_y) + 1
         x * y           S = S_x S_y,    c = c_x + c_y + 1          (an fma: the product and the sum, ONE rounding)
         x / y, y > 0    S = S_x / y + |x / y| (S_y / y),  c = max(c_x, c_y) + 1
                         (|d(x/y)| <= dx / y + |x / y| dy / y, then the quotient's own rounding on |x / y| <= S_x / y)
     A divisor (the pair's distance, a coordinate's modulus) therefore enters with its TRUE value -- a larger one
     would shrink the bound -- and brings its own condition number S_y / y >= 1: the price of the cancellation in q - t.
     For a p-norm y = (sum x_k^p)^(1/p) of non-negative x_k: S_y = sum S_k^p / y^(p-1)  (>= y; p = 1: sum S_k).
  K  the reduction length of the output: m for g_a and g_p, n for g_tgt.  (K - 1) u bounds a float32 sum of K terms in
     ANY order (tree, split-K partials, float atomics), the products of a dot product included, so nothing is measured.
  C  the float32 roundings outside the sum on the longest path to the output; counted below, constant by constant,
     from bwd_gemm.hip (bwdg_build_q_kernel, bwdg_chain_kernel), bwd_device.hpp (transe_w, rotate_w) and bwd.hip
     (bwd_pairs_kernel), pairs_device.hpp for the stored score.  The library is built with -ffp-contract=off and
     IEEE division / square root: one rounding per written operation.

The planted defects of tests/test_pairs_bwd_ref_cpu.py are evaluated by the same code (`defect=`), and the fixed case
lists of tests/test_gpu_pairs_bwd.py are built here (`DOT_CASES`, `DIST_CASES`, `make_case`) so that the CPU file checks
the very inputs the GPU file runs.
"""
import math

import numpy as np

U = 2.0 ** -24

# ---- the counts ------------------------------------------------------------------------------------------------------
C_SINCOS = 2      # sincos_canon (common.hpp): Cody-Waite reduction by fma + degree-7/8 polynomials, |x| <= pi: each of
                  # cos, sin within 2 u ABSOLUTE (S = 1)
C_POW = 2         # powf (device libm): within 2 ulp
# ComplEx q = a r -+ a' r' (bwdg_build_q_kernel / build_q4): product 1 + sum 1;  DistMult q = a r: 1
C_Q = {"complex": 2, "distmult": 1, "transe": 1, "rotate": C_SINCOS + 2}  # transe a +- r: 1; rotate a c - a' s: 2 + 1 + 1
# chain rule dq -> row gradient (bwdg_chain_kernel, the epilogue of bwd_pairs_kernel):
#   complex  dq r +- dq' r': 2        distmult  dq r: 1        transe  dq, -dq: 0 (exact)
#   rotate   g_a = dq c +- dq' s: sincos 2 + product 1 + sum 1 = 4;  g_p = dq' q - dq q': C_Q + product 1 + sum 1
C_CHAIN_A = {"complex": 2, "distmult": 1, "transe": 0, "rotate": C_SINCOS + 2}
C_CHAIN_P = {"complex": 2, "distmult": 1, "transe": 0, "rotate": C_Q["rotate"] + 2}


def _c_weight(name, lp, d):
    """Roundings on the path to one term's weight w(e) (0 for the dot-product scorers: the term is g * t or g * q and
    belongs to the sum).  e = q - t: C_Q + 1."""
    if name in ("complex", "distmult"):
        return 0
    c_e = C_Q[name] + 1  # transe 2, rotate 5
    if name == "transe":
        if lp == 1.0:
            return c_e  # sign(e): exact once the sign is right (the inputs are built so that it is); e's two counted
        if lp == 2.0:
            # stored score (pairs_device.hpp): dist^2 = sum of d fmas, sqrt: (c_e + d/2 + 1) u S_dist;  w = e / dist: + 1
            c_dist = c_e + math.ceil(d / 2) + 1
            return max(c_e, c_dist) + 1
        # dist^p = sum powf(|e|, p) (p c_e + 2 per term, d sums), dist = powf(., 1/p) with 1/p itself rounded:
        # (c_e + (d + 2) / p + 4) u S_dist;  w = powf(|e|, p-1) / powf(dist, p-1) * sign: the powers multiply the operands'
        # relative errors by p - 1, then two powf and the division
        c_dist = c_e + math.ceil((d + 2) / lp) + 4
        return math.ceil((lp - 1) * max(c_e, c_dist)) + 2 * C_POW + 1
    h = d // 2
    c_ab = c_e + 2  # ab = sqrt(fma(e', e', e e)): (product 1 + fma 1) / 2 + sqrt 1, on top of c_e
    if lp == 1.0:
        return max(c_e, c_ab + 1) + 1  # f = 1 / ab: + 1;  w = e * f: + 1
    if lp == 2.0:
        c_dist = c_ab + math.ceil(h / 2) + 1  # dist^2 = sum of h fmas of ab, sqrt
        return max(c_e, c_dist + 1) + 1  # f = 1 / dist: + 1;  w = e * f: + 1
    raise NotImplementedError("bound: rotate with l_norm not in (1, 2)")


def c_counts(name, l_norm, d):
    """(C of g_a, C of g_p, C of g_tgt)"""
    cw = _c_weight(name, float(l_norm), d)
    c_t = cw + (C_Q[name] if name in ("complex", "distmult") else 0)  # dT = G^T Q: the query's own roundings
    return cw + C_CHAIN_A[name], cw + C_CHAIN_P[name], c_t


# ---- gathered operands -------------------------------------------------------------------------------------------------
def _operands(name, ent, rel, a, p, targets, defect, dtype=np.float64):
    ent, rel = np.asarray(ent, dtype), np.asarray(rel, dtype)
    a, p = np.asarray(a).astype(np.int64), np.asarray(p).astype(np.int64)
    if defect.get("rel_next"):  # row i + 1's relation row for row i
        p = np.roll(p, -1)
    A, R = ent[a], rel[p]
    T = ent if targets is None else ent[np.asarray(targets).astype(np.int64)]
    if defect.get("zero_last"):  # the last coordinate (pair) of the target rows read as zero
        T = T.copy()
        d = T.shape[1]
        T[:, d - 1] = 0.0
        if name in ("complex", "rotate"):
            T[:, d // 2 - 1] = 0.0
    return A, R, T


def _masks(G, defect):
    """gout as the m-reduction (g_a, g_p) and as the n-reduction (g_tgt) see it: dropped indices contribute nothing."""
    Gm, Gn = G, G
    if defect.get("drop_m") is not None:
        Gm = G.copy()
        Gm[:, defect["drop_m"]] = 0.0
    if defect.get("drop_n") is not None:
        Gn = G.copy()
        Gn[defect["drop_n"], :] = 0.0
    return Gm, Gn


def _halves(X):
    h = X.shape[1] // 2
    return X[:, :h], X[:, h:]


# ---- ComplEx / DistMult ------------------------------------------------------------------------------------------------
def _dot(name, direction, A, R, T, Gm, Gn, sg, flip=False):
    """sg = -1: the gradients; sg = +1 on magnitudes: the companion (the two directions then coincide)."""
    if name == "distmult":
        dQ, dT = Gm @ T, Gn.T @ (A * R)
        return dQ * R, dQ * A, dT
    (are, aim), (rre, rim) = _halves(A), _halves(R)
    if direction == "sp":  # q = a r
        qre, qim = are * rre + sg * aim * rim, aim * rre + are * rim
    else:  # q = conj(r) a
        qre, qim = rre * are + rim * aim, rre * aim + sg * rim * are
    dT = Gn.T @ np.hstack([qre, qim])
    dre, dim_ = _halves(Gm @ T)
    if direction == "sp":
        f = -sg if flip else sg  # the planted sign flip of one cross term
        ga = np.hstack([dre * rre + dim_ * rim, dim_ * rre + f * dre * rim])
        gp = np.hstack([dre * are + dim_ * aim, dim_ * are + sg * dre * aim])
    else:
        f = -sg if flip else sg
        ga = np.hstack([dre * rre + f * dim_ * rim, dre * rim + dim_ * rre])
        gp = np.hstack([dre * are + dim_ * aim, dre * aim + sg * dim_ * are])
    return ga, gp, dT


# ---- TransE / RotatE: weights of the pairs of a block of query rows ----------------------------------------------------
def _pnorm_w(ae, Se, lp):
    """x = ae >= 0 [n, m, k] with scales Se: dist = ||x||_p over the last axis, its scale, and where it is positive."""
    if lp == 1.0:
        dist, Sd = ae.sum(-1), Se.sum(-1)
    else:
        dist = (ae ** lp).sum(-1) ** (1.0 / lp)
        with np.errstate(divide="ignore", invalid="ignore"):
            Sd = (Se ** lp).sum(-1) / dist ** (lp - 1.0)
    pos = dist > 0
    return np.where(pos, dist, 1.0)[..., None], np.where(pos, Sd, 1.0)[..., None], pos[..., None]


def _transe_w(q, Sq, T, lp, eps):
    e = q[:, None, :] - T[None, :, :] + eps
    Se = Sq[:, None, :] + np.abs(T)[None, :, :]
    if lp == 1.0:
        return np.sign(e), np.ones_like(e)
    ae = np.abs(e)
    dist, Sd, pos = _pnorm_w(ae, Se, lp)
    W = np.where(pos, np.sign(e) * (ae / dist) ** (lp - 1.0), 0.0)
    SW = np.where(pos, (Se / dist) ** (lp - 1.0) + np.abs(W) * (Sd / dist), 0.0)
    return W, SW


def _rotate_w(qre, qim, Sq, T, lp):
    tre, tim = _halves(T)
    ere, eim = qre[:, None, :] - tre[None], qim[:, None, :] - tim[None]
    Sre, Sim = Sq[:, None, :] + np.abs(tre)[None], Sq[:, None, :] + np.abs(tim)[None]
    ab = np.hypot(ere, eim)
    ok = ab > 0
    abs_ = np.where(ok, ab, 1.0)
    Sab = (Sre ** 2 + Sim ** 2) / abs_  # the 2-norm rule on the two components
    if lp == 1.0:
        f, kap = np.where(ok, 1.0 / abs_, 0.0), np.where(ok, Sab / abs_, 0.0)
    else:
        dist, Sd, pos = _pnorm_w(ab, Sab, lp)
        f = np.where(pos & ok, abs_ ** (lp - 2.0) / dist ** (lp - 1.0), 0.0)
        kap = np.where(pos & ok, Sd / dist, 0.0)  # (bound: lp = 2 only)
    wre, wim = ere * f, eim * f
    return wre, wim, Sre * f + np.abs(wre) * kap, Sim * f + np.abs(wim) * kap, ab


def _dist(name, lp, direction, A, R, T, G, Gm, Gn, want_bound, eps=0.0, min_ab=None):
    n, m, d = A.shape[0], T.shape[0], A.shape[1]
    aG, aGm, aGn = np.abs(G), np.abs(Gm), np.abs(Gn)
    dQ, dqA = np.zeros((n, d), A.dtype), np.zeros((n, d))
    dT, dtA = np.zeros((m, d), A.dtype), np.zeros((m, d))
    if name == "rotate":
        (are, aim), cs, sn = _halves(A), np.cos(R), np.sin(R)
        if direction == "sp":
            qre, qim = are * cs - aim * sn, are * sn + aim * cs
        else:
            qre, qim = cs * are + sn * aim, cs * aim - sn * are
        Sq = np.abs(are) + np.abs(aim)
    else:
        q = A + R if direction == "sp" else A - R
        Sq = np.abs(A) + np.abs(R)
    step = max(1, int(2_000_000 // max(1, m * d)))
    for i0 in range(0, n, step):
        s = slice(i0, min(n, i0 + step))
        if name == "rotate":
            wre, wim, swre, swim, ab = _rotate_w(qre[s], qim[s], Sq[s], T, lp)
            if min_ab is not None:
                min_ab.append(float(ab.min()))
            W, SW = np.concatenate([wre, wim], -1), np.concatenate([swre, swim], -1)
        else:
            W, SW = _transe_w(q[s], Sq[s], T, lp, eps)
        # dscore / dq = -w, dscore / dt = +w
        dQ[s] = -np.einsum("ij,ijk->ik", Gm[s], W)
        dT += np.einsum("ij,ijk->jk", Gn[s], W)
        if want_bound:
            dqA[s] = np.einsum("ij,ijk->ik", aGm[s], SW)
            dtA += np.einsum("ij,ijk->jk", aGn[s], SW)
    if name == "transe":
        gp = dQ if direction == "sp" else -dQ
        return (dQ, gp, dT), (dqA, dqA, dtA)
    dre, dim_ = _halves(dQ)
    if direction == "sp":  # q = a (c + i s):  dq/da, dq/dphase = i q
        ga = np.hstack([dre * cs + dim_ * sn, dim_ * cs - dre * sn])
        gp = dim_ * qre - dre * qim
    else:  # q = (c - i s) a:  dq/dphase = -i q
        ga = np.hstack([dre * cs - dim_ * sn, dre * sn + dim_ * cs])
        gp = dre * qim - dim_ * qre
    are_, aim_ = _halves(dqA)
    return (ga, gp, dT), (np.hstack([are_ + aim_, are_ + aim_]), (are_ + aim_) * Sq, dtA)


def _run(name, l_norm, direction, ent, rel, a, p, targets, gout, defect, want_bound, min_ab=None, dtype=np.float64):
    defect = defect or {}
    lp = float(l_norm)
    A, R, T = _operands(name, ent, rel, a, p, targets, defect, dtype)
    G = np.asarray(gout, dtype)
    Gm, Gn = _masks(G, defect)
    if name in ("complex", "distmult"):
        val = _dot(name, direction, A, R, T, Gm, Gn, -1.0, bool(defect.get("flip_cross")))
        comp = _dot(name, direction, np.abs(A), np.abs(R), np.abs(T), np.abs(Gm), np.abs(Gn), 1.0) if want_bound else None
    else:
        val, comp = _dist(name, lp, direction, A, R, T, G, Gm, Gn, want_bound, float(defect.get("eps", 0.0)), min_ab)
    return val, comp


def pairs_bwd(name, l_norm, direction, ent, rel, a, p, targets, gout, defect=None, dtype=np.float64):
    """-> (g_a, g_p, g_tgt) in float64.  `defect`: a planted defect (tests/test_pairs_bwd_ref_cpu.py).  dtype=np.float32:
    the same formulas with every array in float32, in numpy's order -- one more float32 evaluation the bound must hold for."""
    return _run(name, l_norm, direction, ent, rel, a, p, targets, gout, defect, False, None, dtype)[0]


def pairs_bwd_bound(name, l_norm, direction, ent, rel, a, p, targets, gout):
    """-> (b_a, b_p, b_tgt): |float32 result - pairs_bwd| <= bound elementwise (module docstring)."""
    _, comp = _run(name, l_norm, direction, ent, rel, a, p, targets, gout, None, True)
    n = np.asarray(gout).shape[0]
    m = np.asarray(gout).shape[1]
    d = np.asarray(ent).shape[1]
    ca, cp, ct = c_counts(name, l_norm, d)
    return (m + ca) * U * comp[0], (m + cp) * U * comp[1], (n + ct) * U * comp[2]


def rotate_min_modulus(direction, ent, rel, a, p, targets, gout):
    """min |q - t| over every pair and complex coordinate of a RotatE case"""
    acc = []
    _run("rotate", 1.0, direction, ent, rel, a, p, targets, gout, None, False, acc)
    return min(acc)


def transe_ties(direction, ent, rel, a, p, targets):
    """number of (pair, coordinate) with q == t exactly"""
    A, R, T = _operands("transe", ent, rel, a, p, targets, {})
    q = A + R if direction == "sp" else A - R
    return int((q[:, None, :] == T[None, :, :]).sum())


# ---- the host rules restated: how the m-reduction is split (the "last part dropped" defect) and which load path a ------
# ---- product takes (the branch list of DESIGN.md section 21, asserted in tests/test_pairs_bwd_ref_cpu.py) -------------
def gemm_split(M, N, K, scratch_floats):
    """(parts, kc) of run_gemm32 (bwd_gemm32.hip) for C[M, N] over K with `scratch_floats` of scratch"""
    BM = 256 if M > 128 else 128
    tiles = -(-M // BM) * -(-N // 128)
    if not (K > 128 and tiles < 128 and scratch_floats > 0 and (M * N) % 4 == 0):
        return 1, K
    P = min(256 // tiles, scratch_floats // (M * N), K // 64)
    if P < 2:
        return 1, K
    kc = -(-(-(-K // P)) // 32) * 32
    return -(-K // kc), kc


def gemm_vec(lda, ldb, es=4, al=16):
    """`vec` of run_gemm32 on float32 operands whose base addresses are 16-byte aligned (the tests' are): both row
    pitches whole 16-byte pieces.  (es, al) = (2, 8): its `in16` rule, bf16 operands in 8-byte pieces."""
    return int((lda * es) % al == 0 and (ldb * es) % al == 0)


def dot_branches(case):
    """What the two products of a ComplEx / DistMult case run through in gemm32_kernel / run_gemm32, from the host rules:
    {"dq": ..., "dt": ...}, each with vec, BM, parts, kc, nchunk (K chunks of the first part), inner (a tile on the plain
    vector-load path), b_tail (g32_load4 on B with vec = 1 and 1..3 valid elements: N % 4 != 0), a_tail (the same on A:
    a part of dQ whose length is no multiple of 4; for dT, M % 4 != 0)."""
    n, d = case["n"], case["d"]
    listed = case.get("listed")
    m = listed if listed else case["E"]
    ldg = case.get("gout_ld") or m
    out = {}
    for key, M, K, ldb, scratch in (("dq", n, m, d if listed else case.get("ent_ld") or d, 0 if listed else m * d),
                                    ("dt", m, n, d, 0)):
        vec, BM = gemm_vec(ldg, ldb), 256 if M > 128 else 128
        parts, kc = gemm_split(M, d, K, scratch)
        last = K - (parts - 1) * kc
        out[key] = dict(vec=vec, BM=BM, parts=parts, kc=kc, nchunk=-(-min(kc, K) // 32),
                        inner=bool(vec and M >= BM and d >= 128), b_tail=bool(vec and d % 4),
                        a_tail=bool(vec and ((last % 4 or kc % 4) if key == "dq" else M % 4)))
    return out


def pairs_split(n, m, d):
    """(parts, ychunk) of launch_bwd_pairs (bwd.hip): the query-side pass split over blockIdx.z"""
    gc, gr = -(-((d + 1) // 2) // 32), -(-n // 64)
    ys = min(32, 1024 // (gc * gr))
    if ys <= 1:
        return 1, m
    ychunk = -(-(-(-m // ys)) // 16) * 16
    ys = -(-m // ychunk)
    return (ys, ychunk) if ys > 1 else (1, m)


def last_part(case):
    """the indices of the last part of the m-reduction, or None where the reduction is not split"""
    n, m, d = case["n"], case["m"], case["d"]
    if case["name"] in ("complex", "distmult"):
        parts, kc = gemm_split(n, d, m, 0 if case["listed"] else m * d)
    else:
        parts, kc = pairs_split(n, m, d)
    return None if parts < 2 else np.arange((parts - 1) * kc, m)


# ---- the fixed cases ---------------------------------------------------------------------------------------------------
def _dot_case(name, n, E, d, **kw):
    return dict(name=name, l_norm=1.0, n=n, E=E, d=d, **kw)


# (the branch each shape reaches: DESIGN.md, "Pair-score backward against float64")
DOT_CASES = [
    _dot_case("complex", 1, 1, 2),
    _dot_case("distmult", 1, 1, 1),
    _dot_case("complex", 37, 150, 40),
    _dot_case("distmult", 37, 150, 40),
    _dot_case("complex", 128, 256, 128),
    _dot_case("complex", 129, 257, 132),
    _dot_case("complex", 129, 257, 132, gout_ld=260),
    _dot_case("complex", 70, 150, 130, ent_ld=132, gout_ld=152),
    _dot_case("distmult", 70, 150, 130, ent_ld=132, gout_ld=152),
    _dot_case("distmult", 3, 200, 33),
    _dot_case("complex", 130, 200, 40),
    _dot_case("complex", 5, 2177, 8),
    _dot_case("complex", 33, 300, 24),
    _dot_case("distmult", 64, 300, 24),
    _dot_case("complex", 65, 300, 24),
    _dot_case("complex", 16, 1000, 40, listed=300),
    _dot_case("complex", 37, 150, 40, triples32=True),
]


def _dist_case(name, l_norm, d, n, E, **kw):
    return dict(name=name, l_norm=float(l_norm), n=n, E=E, d=d, **kw)


DIST_CASES = [
    _dist_case("transe", 1, 1, 1, 1),
    _dist_case("transe", 1, 2, 63, 15),
    _dist_case("transe", 1, 33, 64, 16),
    _dist_case("transe", 1, 64, 65, 17),
    _dist_case("transe", 1, 66, 130, 150),
    _dist_case("transe", 1, 130, 1, 1037),
    _dist_case("transe", 1, 2, 130, 40, listed=1),
    _dist_case("transe", 2, 33, 65, 150),
    _dist_case("transe", 2, 130, 63, 17),
    _dist_case("transe", 2, 64, 130, 200, listed=150),
    _dist_case("transe", 2, 1, 64, 16),
    _dist_case("transe", 2, 2, 1, 150),
    _dist_case("transe", 3, 66, 63, 150),
    _dist_case("rotate", 1, 2, 1, 1),
    _dist_case("rotate", 1, 64, 63, 15),
    _dist_case("rotate", 1, 66, 64, 16),
    _dist_case("rotate", 1, 130, 65, 17),
    _dist_case("rotate", 1, 2, 130, 150),
    _dist_case("rotate", 1, 64, 1, 1037),
    _dist_case("rotate", 1, 66, 130, 40, listed=1),
    _dist_case("rotate", 2, 66, 65, 150),
    _dist_case("rotate", 2, 130, 63, 16),
    _dist_case("rotate", 2, 64, 130, 200, listed=150),
    _dist_case("rotate", 2, 2, 64, 17),
    _dist_case("rotate", 2, 64, 1, 150),
]

ALL_CASES = DOT_CASES + DIST_CASES


def case_id(c):
    extra = "".join(f"-{k}{'' if v is True else v}" for k, v in c.items()
                    if k not in ("name", "l_norm", "n", "E", "d"))
    norm = "" if c["name"] in ("complex", "distmult") else f"-L{c['l_norm']:g}"
    return f"{c['name']}{norm}-n{c['n']}-E{c['E']}-d{c['d']}{extra}"


def _mag(rng, shape):
    """magnitudes in [0.5, 1] with random signs, rounded to float32: every product of comparable size"""
    return (rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def make_case(c, direction, seed=None):
    """The inputs of one case and direction, float32 / int64 numpy arrays: a dict with the case's fields plus ent [E, d],
    rel [R, d_r], a [n], p [n], targets (None or [m]), gout [n, m], m, listed."""
    name, n, E, d = c["name"], c["n"], c["E"], c["d"]
    if seed is None:
        seed = 1000 * ALL_CASES.index(c) + (0 if direction == "sp" else 1)
    rng = np.random.default_rng(seed)
    R = 7
    dr = d // 2 if name == "rotate" else d
    listed = c.get("listed")
    m = listed if listed else E
    p = rng.integers(0, R, n)
    a = rng.integers(0, E, n)
    targets = None
    if listed:  # with duplicates (listed > 1): every third entry repeats its predecessor's row
        targets = rng.integers(0, E, m)
        targets[2::3] = targets[1::3][: len(targets[2::3])]
    if name in ("complex", "distmult"):
        ent, rel = _mag(rng, (E, d)), _mag(rng, (R, dr))
    elif name == "transe":
        # a dyadic grid: multiples of 2^-6 in [-2, 2] -- a + r - t is exact in float32 and in float64, so every sign agrees
        ent = (rng.integers(-128, 129, (E, d)) / 64.0).astype(np.float32)
        rel = (rng.integers(-128, 129, (R, dr)) / 64.0).astype(np.float32)
        if E == 1:  # the query's own row is the only target, q - t = +-r: a row that outweighs it, so that a target read
            ent[:], rel[:] = 1.5, (-0.5 if direction == "sp" else 0.5)  # as zero changes the sign of q - t
        # exact ties q == t in the first half of the coordinates of pair (0, j0): j0 a target row that is not a[0]'s
        tid = np.arange(E) if targets is None else targets
        other = np.nonzero(tid != a[0])[0]
        half = slice(0, (d + 1) // 2)
        if other.size:
            q0 = ent[a[0]] + rel[p[0]] if direction == "sp" else ent[a[0]] - rel[p[0]]
            ent[tid[other[0]], half] = q0[half]
        else:  # the query's own row is the only target: q - t = +-r (d = 1: no tie, the one coordinate stays)
            rel[p[0], : d // 2] = 0.0
    else:
        # moduli per complex coordinate: the (at most 4) rows used by queries on four levels below 0.72, every other row
        # in [1, 1.5] -- |q - t| >= | |q| - |t| | >= 0.04 between different rows, 0.28 for all but the four (a small
        # |q - t| is a large condition number of the weight, and the bound grows with it); phases with
        # 0.1 <= |r| <= pi, so that a query row met as its own target stays 0.05 away
        nq = min(4, E)
        a = rng.integers(0, nq, n)
        mod = rng.uniform(1.0, 1.5, (E, d // 2))
        mod[:nq] = 0.5 + 0.06 * np.arange(nq)[:, None] + rng.uniform(0.0, 0.02, (nq, d // 2))
        ang = rng.uniform(-np.pi, np.pi, (E, d // 2))
        ent = np.hstack([mod * np.cos(ang), mod * np.sin(ang)]).astype(np.float32)
        rel = (rng.uniform(0.1, 3.14, (R, dr)) * rng.choice([-1.0, 1.0], (R, dr))).astype(np.float32)
    gout = _mag(rng, (n, m))
    out = dict(c)
    out.update(direction=direction, ent=ent, rel=rel, a=a.astype(np.int64), p=p.astype(np.int64),
               targets=None if targets is None else targets.astype(np.int64), gout=gout, m=m, listed=bool(listed))
    return out


def ref_args(k):
    return (k["name"], k["l_norm"], k["direction"], k["ent"], k["rel"], k["a"], k["p"], k["targets"], k["gout"])
