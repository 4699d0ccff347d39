"""The fused float32 losses of the DISTANCE scorers (kge_ce_dist_*, kge_kl_dist_*, kge_bce_dist_*: ce_dist.hip, TransE /
RotatE) and of float32 ComplEx / DistMult tables (kge_ce_f32_*, kge_kl_f32_*, kge_bce_f32_*: ce_f32.hip and the fold /
gradient epilogues of score_pairs_f32.hip) restated in numpy float64 for the tests (no torch, no GPU), with elementwise
bounds counted from the source.  The text below counts the distance family line by line; THE F32 FAMILY at its end lists
what differs.  The
gradient closed forms, the companion values, `U` and the counts `c_counts` are those of _pairs_bwd_ref.py.

SCORES      The float32 score bits of the family are canonical: kge_score_sp / kge_score_po equal oracle.score_sp /
            score_po bit for bit (asserted by tests/test_gpu_ce_dist.py and again by tests/test_gpu_dense32_bound.py), and
            ce_dist_fwd_kernel folds the tile pairs_kernel stores (ce_dist.hip:229-233).  Every bound below therefore starts
            from the oracle's bits x, computed on the CPU; no score-accumulation term exists.  The label scores carry the
            stored bits too (the CE record ce_dist.hip:267-273, dist_label_score :349-375): the loss bounds have no score
            term, and a label score with other bits shows as a ratio above 1.

ASSUMPTION ABOUT libm.  C_TR = 2 (units of u = 2^-24): the device libm documents expf, logf and log1pf of float32 at 1 ulp
            (2 u); taken from the documentation, never fitted to a kernel's output.  A result below 2^-126 may come out as
            zero (FLUSH: every bound carries a term for it).  Float32 division (the sigmoid, 1 / k_i) is correctly rounded:
            the library is built without fast math.  A ratio above 1 in tests/test_gpu_dense32_bound.py is a finding about a
            kernel or about C_TR, told apart by the float32 restatements below (`fwd_restated`, `coef_restated`).

FORWARD     lse of a row from its bits x (X = max |x|, rng = max x - min x, m columns, T = col_tiles walked tiles per
            workgroup, G column groups: `cd_groups`).  Every sum is a sum of positive terms: a term's relative error is
            bounded by the roundings on ITS path.  rho, in units of u:
              rng          the exponent v[k] - nm (ce_dist.hip:263): one rounding, at most u rng
              C_TR         expf of the term (:263)
              16           the additions of one fold step (:262-263): a term passes at most 16
              (T - 1)(C_TR + 17)   one rescale per later walked tile, run_s * expf(run_m - nm) (:260): expf, the product,
                           and the 16 additions of that step
              rng          the exponents run_m - nm of those rescales telescope to at most the range
              rng + C_TR + 5       the merge of the row's four threads (:298): subtraction, expf, product, four additions
              rng + C_TR + 1 + G   the serial merge of the G records (ce_dist_merge_kernel :320, ml_dist_finish_kernel :428)
            b_lse = rho (1 + rho) + C_TR u log m  [logf(ss), ss in [1, m]] + u (X + log m)  [mm + logf(ss) :321 / :429]
                    + FLUSH: 2 m (T + 3) 2^-126
            ce    loss = l - record (:325): b_lse + u |loss|
            kl    the label scores in CSR order through __shfl (:411): (k - 1) u sum |x|; sum / k, logf(k) and two
                  subtractions (:433), or w * sum and one subtraction (:432)
            bce   softplus_f (:135-137) per term: u |x + off| (the addition :252; softplus is 1-Lipschitz) + C_TR u e
                  (expf, e = exp(-|x + off|); log1p is 1-Lipschitz) + C_TR u log1p(e) (log1pf) + u sp (the fmaxf addition)
                  + 2^-126; a term passes at most 16 T + 4 + G additions (:252, :288, :419); the label sum
                  u |x + off| per entry (:406) + (k - 1) u sum |x + off| (:411), and the subtraction (:420)

GRADIENT COEFFICIENTS.  kge_*_dist_bwd takes lse as an input: the reference takes the same float32 vector, no forward
            error enters.  From the bits x in float64 (`coef64`):
              ce   p = g_i (exp(x - lse_i) - [j = label_i])
              kl   p = g_i (exp(x - lse_i) - w_i [j in labels_i])
              bce  p = g_i (sigmoid(x + offset) - [j in labels_i])
            with g_i, w_i as ml_rows_kernel writes them (:764-780: w_i = label_weight_i or fl(1 / k_i); g_i = 0 for a row
            without labels under unweighted kl).  The `weight` lambda (:583-598) stays inside [p - e, p + e] (`coef_radius`):
              exp   w = expf(s - lse_i): the subtraction u |s - lse|, expf C_TR u, both relative to w; or zero below 2^-126
              sig   z = s + offset: u |z|; expf(-z): C_TR u; 1 + e and 1 / (.): u each -> (1 - sig)(|z| + C_TR) u + 2 u
                    relative to sig; + 2^-126 where expf overflows or flushes
              label w - 1, w - w_i: u |w - .|
              g * w one rounding u |p|, + 2^-149

GRADIENTS   _pairs_bwd_ref.pairs_bwd on the coefficient matrix p.  Bound = pairs_bwd_bound on |p| + e -- (K + C) u A with
            K = E for g_a / g_p and n for g_tgt -- plus the companion value of e itself (e pushed through the same closed
            forms).  C recounted for the kernels that run: ce_dist_bwd_kernel takes e = q - t from build_q4 and the streamed
            row (:659-660), the distance from the stored chunk (dist = -s :597, the score's own roundings, counted by
            _c_weight), transe_w / rotate_w of bwd_device.hpp (:663-669), and accumulates by fma (one rounding per term:
            inside K); ce_dist_chain_kernel (:700-737) is the epilogue of bwd_pairs_kernel.  The counts are therefore
            c_counts' own.  The (K - 1) u any-order term of _pairs_bwd_ref covers the float atomics across blockIdx.z
            (:691) and the chunk order: nothing is measured.

INPUTS      `make_case`: TransE tables on the dyadic grid 2^-6, so that q = a +- r and q - t are exact in float32 -- every L1
            sign is decided and an exact zero difference is an exact zero in both precisions.  RotatE rows have moduli
            M + delta >= 1 and phases in [0.1, pi - 0.1]: |q - t| stays away from zero except where a zero is planted.

THE F32 FAMILY.  The same fold on another geometry (`geometry`): 128-column tiles, TWO threads per row, FOUR 16-column
            steps per thread and tile (score_pairs_f32.hip:210-248), so a thread takes S = 4 T steps: the FORWARD count
            reads (S - 1)(C_TR + 17) and the lane merge C_TR + 1 + 2 (:319-323); bce depth 16 S + 2 + G (:225, :317,
            ce_f32.hip:310); groups by cf_groups (ce_f32.hip:69-80), records merged by ce_dist_merge_kernel with
            col_tiles * 2.  The scores inside the folds are kge_score_sp / kge_score_po's bits (the oracle's).  The LABEL
            SCORES of kl / bce are not: ml_f32_finish_kernel (ce_f32.hip:290-296) takes <Q_i, T_j> as one fmaf chain over
            d coordinates of a query built with C_Q roundings -- the reference takes the exact float64 <Q_i, T_j> and the
            bound (d + C_Q) u (|Q_i| . |T_j|) per label (`label_scores64`).  COEFFICIENTS: F3_GRAD / F3_GRAD_BCE are the
            `weight` lambda's expressions (:258-270, :283-285); F3_GRAD_KL subtracts label_bias first,
            p = g_i (exp(x - lse_i) - b_i - w_i [j in labels_i]): one more rounding u |exp - b_i| (:283).  The padding
            columns of a G block are exactly zero (:268, :285).  GRADIENTS: dT = G^T Q and dQ = G T are two run_gemm32
            products, the split-K partials and the chunks are summed by ce_f32_dq_sum_kernel (ce_f32.hip:168-181: inside
            the any-order K term), the chain rule is bwdg_chain_kernel: the route of kge_score_pairs_bwd, so C is
            c_counts' (C_Q for g_tgt, C_CHAIN for g_a / g_p).  INPUTS (`make_case_f32`): entity rows pr_j amp w + noise
            orthogonal to w, relation 0 exactly one, so that a hot row scores TARGET pr_j.

The fixed case lists (`CASES_DIST`, `CASES_F32`, each case with its `why`), the host rules (`cd_groups`, `cf_groups`) and the planted defects (`defect=`) are
here so that tests/test_dense32_ref_cpu.py checks the very inputs tests/test_gpu_dense32_bound.py runs.
"""
import math

import numpy as np

import _pairs_bwd_ref as R
from _pairs_bwd_ref import U, c_counts  # noqa: F401

C_TR = 2
TINY = 2.0 ** -126
SUB = 2.0 ** -149
PT = 64        # PT_BM = PT_BN (pairs_device.hpp)
GRID = 64.0    # the dyadic grid of the TransE tables: multiples of 2^-6


# ---- the host rule -----------------------------------------------------------------------------------------------------
F32 = ("complex", "distmult")


def geometry(name):
    """(tile width, fold threads per row, 16-column fold steps per thread and tile): ce_dist_fwd_kernel 64 / 4 / 1,
    pairs_f32_kernel's fold epilogue 128 / 2 / 4 (score_pairs_f32.hip:207-249, :306-329)"""
    return (128, 2, 4) if name in F32 else (PT, 4, 1)


def groups(name, n, m):
    """(col_tiles, groups): cd_groups (ce_dist.hip) on 64-wide tiles, cf_groups (ce_f32.hip) on 128-wide tiles"""
    tw = geometry(name)[0]
    rg, tiles = -(-n // tw), -(-m // tw)
    want = max(1, min(1024 // max(rg, 1), 256, tiles))
    ct = max(1, -(-tiles // want))
    return ct, max(1, -(-tiles // ct))


def cd_groups(n, m):
    return groups("transe", n, m)


def cf_groups(n, m):
    return groups("complex", n, m)


def records_bytes(n, m, name="transe"):
    return -(-(n * groups(name, n, m)[1] * 12) // 256) * 256


# ---- float64 forward ---------------------------------------------------------------------------------------------------
def lse64(x):
    x = np.asarray(x, np.float64)
    mx = x.max(axis=1)
    return mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))


def csr_rows(k):
    rp, col = k["rowptr"], k["col"]
    return [col[rp[i]:rp[i + 1]] for i in range(len(rp) - 1)]


def _rho(x, n, name):
    x = np.asarray(x, np.float64)
    m = x.shape[1]
    T, G = groups(name, n, m)
    _, nt, spt = geometry(name)
    S = T * spt  # fold steps of one thread
    rng = x.max(axis=1) - x.min(axis=1)
    return U * (4 * rng + C_TR + 16 + (S - 1) * (C_TR + 17) + (C_TR + 1 + nt) + (C_TR + 1 + G)), S, G


def lse_bound(x, n, name="transe"):
    """|kernel lse - lse64(x)| for the score bits x of n query rows (module docstring, FORWARD)"""
    x = np.asarray(x, np.float64)
    m = x.shape[1]
    rho, S, _ = _rho(x, n, name)
    X = np.abs(x).max(axis=1)
    return rho * (1 + rho) + C_TR * U * np.log(m) + U * (X + np.log(m)) + 2 * m * (S + 3) * TINY


# ---- the label scores of kl / bce ----------------------------------------------------------------------------------------
def q64(k, mag=False):
    """the query vectors [n, d] of a ComplEx / DistMult case in float64 (mag: the companion, magnitudes and sums)"""
    A, Rr = k["ent"][k["a"]].astype(np.float64), k["rel"][k["p"]].astype(np.float64)
    sg = -1.0
    if mag:
        A, Rr, sg = np.abs(A), np.abs(Rr), 1.0
    if k["name"] == "distmult":
        return A * Rr
    h = A.shape[1] // 2
    are, aim, rre, rim = A[:, :h], A[:, h:], Rr[:, :h], Rr[:, h:]
    if k["direction"] == "sp":
        return np.hstack([are * rre + sg * aim * rim, aim * rre + are * rim])
    return np.hstack([rre * are + rim * aim, rre * aim + sg * rim * are])


def label_scores64(k, x):
    """per row: (the label scores the loss terms are taken from, their bound against the kernel's).  Distance family: the
    stored bits, bound 0 (dist_label_score).  f32 family: the exact <Q_i, T_j>, and (d + C_Q) u (|Q_i| . |T_j|) for
    ml_f32_finish_kernel's fmaf chain over d coordinates of a query with C_Q roundings (ce_f32.hip:290-296)"""
    x = np.asarray(x, np.float64)
    rows = csr_rows(k)
    if k["name"] not in F32:
        return [x[i, js] for i, js in enumerate(rows)], [np.zeros(len(js)) for js in rows]
    Q, Qm, T = q64(k), q64(k, True), k["ent"].astype(np.float64)
    c = (k["d"] + R.C_Q[k["name"]]) * U * (1 + 2.0 ** -10)
    return [Q[i] @ T[js].T for i, js in enumerate(rows)], [c * (Qm[i] @ np.abs(T[js]).T) for i, js in enumerate(rows)]


def loss64(k, x):
    """(loss_rows, lse or None) in float64 from the score matrix x"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    if k["kind"] == "bce":
        xo = x + float(k["offset"])
        loss = (np.maximum(xo, 0) + np.log1p(np.exp(-np.abs(xo)))).sum(axis=1)
        for i, xl in enumerate(label_scores64(k, x)[0]):
            loss[i] -= (xl + float(k["offset"])).sum()
        return loss, None
    z = lse64(x)
    if k["kind"] == "ce":
        return z - x[np.arange(n), k["label"]], z
    loss = np.zeros(n)
    for i, xl in enumerate(label_scores64(k, x)[0]):
        if k.get("label_weight") is not None:
            loss[i] = z[i] - float(k["label_weight"][i]) * xl.sum()
        elif len(xl):
            loss[i] = z[i] - xl.mean() - np.log(len(xl))
    return loss, z


def loss_bound(k, x):
    """bound of loss64's loss rows against the kernel's (module docstring, FORWARD)"""
    x = np.asarray(x, np.float64)
    n, m = x.shape
    loss, z = loss64(k, x)
    xls, bls = label_scores64(k, x) if k["kind"] != "ce" else (None, None)
    if k["kind"] == "bce":
        T, G = groups(k["name"], n, m)
        _, nt, spt = geometry(k["name"])
        xo = x + float(k["offset"])
        e = np.exp(-np.abs(xo))
        sp = np.maximum(xo, 0) + np.log1p(e)
        per = U * np.abs(xo) + C_TR * U * e + C_TR * U * np.log1p(e) + U * sp + TINY
        depth = 16 * T * spt + nt + G
        b = per.sum(axis=1) + depth * U * sp.sum(axis=1) * (1 + depth * U)
        for i, (xl, bl) in enumerate(zip(xls, bls)):
            t = np.abs(xl + float(k["offset"])).sum()
            b[i] += bl.sum() + U * t + max(len(xl) - 1, 0) * U * t + U * abs(loss[i])
        return b
    b = lse_bound(x, n, k["name"])
    if k["kind"] == "ce":
        return b + U * np.abs(loss)
    for i, (js, bl) in enumerate(zip(xls, bls)):
        t = np.abs(js).sum()
        s = max(len(js) - 1, 0) * U * t + bl.sum()
        if k.get("label_weight") is not None:
            w = abs(float(k["label_weight"][i]))
            b[i] += w * s + U * w * t + U * abs(loss[i])
        elif len(js):
            kk = len(js)
            b[i] += s / kk + U * t / kk + C_TR * U * np.log(kk) + U * (abs(z[i]) + t / kk) + U * abs(loss[i])
        else:
            b[i] = 0.0
    return b


# ---- gradient coefficients ---------------------------------------------------------------------------------------------
def row_gradients(k):
    """(g [n], w [n]) float32 as ml_rows_kernel writes them (ce: g_rows / g_scalar, w unused)"""
    n = k["n"]
    g = np.full(n, np.float32(k["g_scalar"]), np.float32) if k.get("g_rows") is None else k["g_rows"].astype(np.float32)
    w = np.ones(n, np.float32)
    if k["kind"] == "kl":
        cnt = np.diff(k["rowptr"])
        if k.get("label_weight") is not None:
            w = k["label_weight"].astype(np.float32)
        else:
            w = np.where(cnt > 0, np.float32(1) / np.maximum(cnt, 1).astype(np.float32), np.float32(1)).astype(np.float32)
            g = np.where(cnt == 0, np.float32(0), g).astype(np.float32)
    return g, w


def label_matrix(k, m):
    y = np.zeros((k["n"], m), bool)
    if k["kind"] == "ce":
        y[np.arange(k["n"]), k["label"]] = True
    else:
        y[np.repeat(np.arange(k["n"]), np.diff(k["rowptr"])), k["col"]] = True
    return y


def coef64(k, x, lse, w=None):
    """p [n, m] in float64 from the scores x and the lse vector the backward is given (unused for bce); w: the label
    weights in place of the float32 values of row_gradients (the autograd comparison: 1 / k_i unrounded)"""
    x = np.asarray(x, np.float64)
    g32, w32 = row_gradients(k)
    g, w = g32.astype(np.float64)[:, None], (w32.astype(np.float64) if w is None else np.asarray(w, np.float64))[:, None]
    y = label_matrix(k, x.shape[1])
    if k["kind"] == "bce":
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-(x + float(k["offset"]))))
        return g * (s - y)
    e = np.exp(x - np.asarray(lse, np.float64)[:, None])
    if k.get("label_bias") is not None:  # F3_GRAD_KL: label smoothing's uniform term
        e = e - k["label_bias"].astype(np.float64)[:, None]
    return g * (e - (w * y if k["kind"] == "kl" else y))


def coef_radius(k, x, lse):
    """e [n, m]: the `weight` lambda of ce_dist_bwd_kernel lies in [p - e, p + e] (module docstring)"""
    x = np.asarray(x, np.float64)
    g32, w32 = row_gradients(k)
    ag, w = np.abs(g32.astype(np.float64))[:, None], w32.astype(np.float64)[:, None]
    y = label_matrix(k, x.shape[1])
    one = 1 + 2.0 ** -10  # second-order terms
    p = coef64(k, x, lse)
    if k["kind"] == "bce":
        z = x + float(k["offset"])
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-z))
        ew = s * ((1 - s) * (np.abs(z) + C_TR) + 2) * U * one + TINY
        ew = ew + np.where(y, U * np.abs(s - 1), 0.0)
    else:
        t = x - np.asarray(lse, np.float64)[:, None]
        wv = np.exp(t)
        ew = wv * (np.abs(t) + C_TR) * U * one + TINY
        if k.get("label_bias") is not None:  # expf(.) - b_i: one more rounding (score_pairs_f32.hip:283)
            wv = wv - k["label_bias"].astype(np.float64)[:, None]
            ew = ew + U * np.abs(wv)
        ew = ew + np.where(y, U * np.abs(wv - (w if k["kind"] == "kl" else 1.0)), 0.0)
    return ag * ew * one + U * np.abs(p) + SUB


# ---- gradients ---------------------------------------------------------------------------------------------------------
def _args(k, gout):
    return (k["name"], k["l_norm"], k["direction"], k["ent"], k["rel"], k["a"], k["p"], None, gout)


def grads(k, P, defect=None):
    """(g_a, g_p, g_tgt) in float64 from a coefficient matrix.  defect {"zero_w1": True}: the weight of a pair at distance
    exactly zero taken as 1 in every coordinate instead of 0 (g_tgt only: the other two are returned unchanged)"""
    if defect and defect.get("pad_one"):  # the first pad column of G holds 1.0 and meets the clamped last target row
        k2 = dict(k, ent=np.vstack([k["ent"], k["ent"][-1:]]))
        ga, gp, gt = R.pairs_bwd(*_args(k2, np.hstack([np.asarray(P, np.float64), np.ones((k["n"], 1))])))
        return ga, gp, gt[:-1]
    ga, gp, gt = R.pairs_bwd(*_args(k, P))
    if defect and defect.get("zero_w1"):
        gt = gt.copy()
        P = np.asarray(P, np.float64)
        for i, j in zip(*np.nonzero(k["zero_pairs"])):
            gt[j] += P[i, j]
    return ga, gp, gt


def grads_and_bound(k, P, E_):
    """-> ((g_a, g_p, g_tgt), (b_a, b_p, b_tgt)) (module docstring, GRADIENTS)"""
    want = grads(k, P)
    acc = R.pairs_bwd_bound(*_args(k, np.abs(P) + E_))
    slack = R.pairs_bwd_companion(*_args(k, E_))
    return want, tuple(a + s * (1 + 16 * U) for a, s in zip(acc, slack))


# ---- float32 restatements (numpy; expf / logf / log1pf correctly rounded: inside C_TR) ----------------------------------
def _f(fn, v):
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        return fn(np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


def q32(k):
    """the query vectors [n, d] in float32 (bwdg_build_q_kernel's products and sums, numpy's roundings: inside C_Q)"""
    A, Rr = k["ent"][k["a"]].astype(np.float32), k["rel"][k["p"]].astype(np.float32)
    if k["name"] == "distmult":
        return A * Rr
    h = A.shape[1] // 2
    are, aim, rre, rim = A[:, :h], A[:, h:], Rr[:, :h], Rr[:, h:]
    if k["direction"] == "sp":
        return np.hstack([are * rre - aim * rim, aim * rre + are * rim])
    return np.hstack([rre * are + rim * aim, rre * aim - rim * are])


def label_scores32(k, x32):
    """per row, float32: the stored bits (distance family) or ml_f32_finish_kernel's fmaf chain over coordinates 0 .. d - 1"""
    rows = csr_rows(k)
    if k["name"] not in F32:
        return [x32[i, js] for i, js in enumerate(rows)]
    Q, T = q32(k).astype(np.float64), k["ent"].astype(np.float64)
    out = []
    for i, js in enumerate(rows):
        sc = np.zeros(len(js), np.float32)
        for c in range(k["d"]):
            sc = (Q[i, c] * T[js, c] + sc.astype(np.float64)).astype(np.float32)
        out.append(sc)
    return out


def fwd_restated(k, x32, defect=None):
    """(loss_rows, lse or None) float32 by the arithmetic of the fold (ce_dist_fwd_kernel: four threads per row, one
    16-column step per tile; pairs_f32_kernel: two threads per row, four steps per 128-column tile), the walk over
    col_tiles tiles, the lane merge, and ce_dist_merge_kernel / ml_dist_finish_kernel / ml_f32_finish_kernel.  `defect`:
      no_rescale_step  the factor expf(run_m - nm) dropped at every fold step after a thread's first
      no_rescale_walk  the factor dropped at the first step of the second walked tile on
      no_rescale_lane  the factor expf(pm - mm) dropped in the merge of the row's threads
      no_pad           the padding test missing: the ragged tile's padding columns (the clamped last row) take part
      pad_00           a thread that saw only padding merged as (max 0, sum 0), without the `> 0` test
      label_group      ce: the label record read from group label / 64 (right only where one 64-wide tile is a group)
      no_offset        bce: the offset ignored"""
    defect = defect or {}
    x = np.asarray(x32, np.float32)
    n, m = x.shape
    T, G = groups(k["name"], n, m)
    tw, nt, spt = geometry(k["name"])
    kind = k["kind"]
    off = np.float32(0.0 if defect.get("no_offset") or kind != "bce" else k["offset"])
    xp = np.repeat(x[:, m - 1:m], G * T * tw, axis=1)
    xp[:, :m] = x
    xp = xp.reshape(n, G, T, nt, spt, 16)
    col = np.arange(G * T * tw).reshape(G, T, nt, spt, 16)
    # (no_pad: whole tiles beyond the table are still skipped -- the col0 >= m break)
    ok = (col // tw * tw) < m if defect.get("no_pad") else col < m
    run_m = np.full((n, G, nt), -np.inf, np.float32)
    run_s = np.zeros((n, G, nt), np.float32)
    seen = np.zeros((G, nt), bool)
    xl = label_scores32(k, x) if kind != "ce" else None
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for t, q16 in ((t, q) for t in range(T) for q in range(spt)):
            v, o = xp[:, :, t, :, q16], ok[None, :, t, :, q16]
            live = o[0, :, :, 0]  # [G, nt]: the thread has a valid column in this step
            if kind == "bce":
                s = run_s.copy()
                for c in range(16):
                    z = v[..., c] + off
                    sp = np.maximum(z, np.float32(0)) + _f(np.log1p, _f(np.exp, -np.abs(z)))
                    s = np.where(o[..., c], s + sp, s)
                run_s = s
            else:
                tm = np.where(o, v, -np.inf).max(axis=-1)
                nm = np.maximum(run_m, tm)
                f = _f(np.exp, run_m - nm)
                if (defect.get("no_rescale_walk") and t > 0 and q16 == 0) or defect.get("no_rescale_step"):
                    f = np.where(np.isinf(run_m), f, np.float32(1))
                s = np.where(np.isinf(nm), np.float32(0), run_s * f)
                for c in range(16):
                    s = np.where(o[..., c], s + _f(np.exp, v[..., c] - nm), s)
                run_m = np.where(live[None], nm, run_m)
                run_s = np.where(live[None], s, run_s)
            seen |= live
        if kind == "bce":
            rec = run_s[..., 0]
            for q in range(1, nt):
                rec = rec + run_s[..., q]
            tot = np.zeros(n, np.float32)
            for g in range(G):
                tot = tot + rec[:, g]
            loss = np.zeros(n, np.float32)
            for i, sc in enumerate(xl):
                sm = np.float32(0)
                for v_ in sc:
                    sm = sm + (v_ + off)
                loss[i] = tot[i] - sm
            return loss, None
        pm, ps = run_m, run_s
        if defect.get("pad_00"):
            pm = np.where(seen[None], pm, np.float32(0))
        mm = pm.max(axis=-1)
        ss = np.zeros((n, G), np.float32)
        for q in range(nt):
            f = np.ones((n, G), np.float32) if defect.get("no_rescale_lane") else _f(np.exp, pm[..., q] - mm)
            add = ps[..., q] * f
            take = np.ones((n, G), bool) if defect.get("pad_00") else ps[..., q] > 0
            ss = np.where(take, ss + add, ss)
        # the serial merge of the records
        live = ss > 0
        M = np.where(live, mm, -np.inf).max(axis=1)
        S = np.zeros(n, np.float32)
        for g in range(G):
            S = np.where(live[:, g], S + ss[:, g] * _f(np.exp, mm[:, g] - M), S)
        z = M + _f(np.log, S)
    if kind == "ce":
        lab = k["label"]
        grp = lab // 64 if defect.get("label_group") else lab // tw // T
        recl = np.zeros((n, G), np.float32)
        recl[np.arange(n), lab // tw // T] = x[np.arange(n), lab]
        flat = np.concatenate([recl.ravel(), np.zeros(m, np.float32)])
        return z - flat[np.arange(n) * G + grp], z
    loss = np.zeros(n, np.float32)
    for i, sc in enumerate(xl):
        sm = np.float32(0)
        for v_ in sc:
            sm = sm + v_
        if k.get("label_weight") is not None:
            loss[i] = z[i] - np.float32(k["label_weight"][i]) * (sm if len(sc) else np.float32(0))
        elif len(sc):
            kk = np.float32(len(sc))
            loss[i] = z[i] - sm / kk - _f(np.log, kk)
    return loss, z


def coef_restated(k, x32, lse32, defect=None, chunk=None):
    """the coefficient matrix [n, m] float32 by the arithmetic of ce_dist_bwd_kernel's `weight` / of F3_GRAD, F3_GRAD_KL,
    F3_GRAD_BCE (score_pairs_f32.hip:258-288); chunk: the smallest chunk width of the family (64 / 128).  `defect`:
      no_bias       f32 kl: label_bias ignored
      label_plus1   ce: the label subtracted at column label + 1
      g_next        g_i (and w_i) of row i + 1
      chunk_last    the last column of every `chunk`-wide chunk dropped (its weight staged as zero)
      mask_word     kl / bce: the label bit read from the neighbouring 32-bit word of the chunk's mask
      no_w          kl: w_i ignored (taken as 1)
      no_offset     bce: the offset ignored
      unlabelled    unweighted kl: g_i of a row without labels not zeroed"""
    defect = defect or {}
    chunk = chunk or geometry(k["name"])[0]
    x = np.asarray(x32, np.float32)
    n, m = x.shape
    g, w = row_gradients(k)
    if defect.get("unlabelled"):
        g = (np.full(n, np.float32(k["g_scalar"]), np.float32) if k.get("g_rows") is None else k["g_rows"].astype(np.float32))
    if defect.get("no_w"):
        w = np.ones(n, np.float32)
    if defect.get("g_next"):
        g, w = np.roll(g, -1), np.roll(w, -1)
    y = label_matrix(k, m)
    if defect.get("label_plus1"):
        y = np.roll(y, 1, axis=1)
        y[:, 0] = False
    if defect.get("mask_word"):
        cols = np.arange(m)
        src = (cols % chunk ^ 32) + cols // chunk * chunk  # bit y & 31 of word (y >> 5) ^ 1
        y = np.where((src < m)[None, :], y[:, np.minimum(src, m - 1)], False)
    if k["kind"] == "bce":
        off = np.float32(0.0 if defect.get("no_offset") else k["offset"])
        wv = np.float32(1) / (np.float32(1) + _f(np.exp, -(x + off)))
        wv = np.where(y, wv - np.float32(1), wv)
    else:
        wv = _f(np.exp, x - np.asarray(lse32, np.float32)[:, None])
        if k.get("label_bias") is not None and not defect.get("no_bias"):
            wv = wv - k["label_bias"].astype(np.float32)[:, None]
        wv = np.where(y, wv - (w[:, None] if k["kind"] == "kl" else np.float32(1)), wv)
    with np.errstate(under="ignore"):
        P = (g[:, None] * wv).astype(np.float32)
    if defect.get("chunk_last"):
        P[:, chunk - 1::chunk] = 0.0
    return P


# ---- the fixed cases ---------------------------------------------------------------------------------------------------
WALK_DIST = (8, PT * 513 + 1, 70)  # (d, E, n): 514 tiles, col_tiles 3, 172 groups, the last one tile with one valid column
LABEL_COLS = (0, 15, 16, 63, 64, 127, 128)
BASE, FAR, SPAN = 101.0, 110.0, 40.0


def _c(name, l_norm, kind, shape, profile, why, **kw):
    d, E, n = shape
    return dict(name=name, l_norm=float(l_norm), kind=kind, d=d, E=E, n=n, profile=profile, why=why, **kw)


GEO, FULL, ONE, RAG1, ODD = (40, 150, 37), (64, 64, 64), (32, 70, 1), (64, PT * 14 + 1, 130), (33, 150, 37)
CASES_DIST = [
    _c("transe", 1, "ce", GEO, "ascending", "ragged everywhere, three tiles: the max rises in every tile"),
    _c("transe", 2, "kl", GEO, "descending", "kl, the max in the first fold step"),
    _c("rotate", 1, "bce", GEO, "spike_first", "bce with an offset, |score| >= 100"),
    _c("rotate", 2, "ce", GEO, "plateau", "five identical target rows: lse = x + log 5", g_scalar=0.25),
    _c("transe", 2, "bce", FULL, "descending", "exactly one full tile, no padding anywhere", g_scalar=-0.5),
    _c("rotate", 1, "klw", FULL, "ascending", "weighted kl on one full tile"),
    _c("transe", 1, "ce", ONE, "spike_last", "one row; the second tile has 6 valid columns: three threads all padding"),
    _c("rotate", 2, "kl", ONE, "spike_first", "one row, unweighted kl: every entity a label", g_scalar=1.5),
    _c("transe", 1, "klw", RAG1, "spike_last", "the last tile has ONE valid column and holds the row maximum"),
    _c("rotate", 2, "ce", RAG1, "spike_last", "the same for RotatE L2, three row groups"),
    _c("rotate", 1, "bce", RAG1, "plateau", "bce over 15 tiles, ties"),
    _c("transe", 1, "ce", ODD, "zero", "d = 33: the unvectorised path; a target equal to the query, sign(0)"),
    _c("transe", 2, "ce", ODD, "zero", "d = 33; a target equal to the query, the L2 weight 0 / 0"),
    _c("rotate", 1, "kl", GEO, "zero", "a zero modulus in every coordinate: 1 / ab guarded"),
    _c("rotate", 2, "bce", GEO, "zero", "zero distance under bce"),
    _c("transe", 1, "ce", WALK_DIST, "spike_tile2", "walk: the maximum arrives in the second walked tile", directions=("sp",)),
    _c("transe", 2, "kl", WALK_DIST, "ascending", "walk: the max rises in every walked tile", directions=("po",)),
    _c("transe", 1, "bce", WALK_DIST, "descending", "walk: the bce record summed across walked tiles", directions=("po",)),
    _c("rotate", 2, "ce", WALK_DIST, "ascending", "walk, RotatE: the max rises in every walked tile", directions=("po",)),
    _c("rotate", 1, "klw", WALK_DIST, "spike_last", "walk: the maximum in the short last group", directions=("sp",)),
    _c("rotate", 2, "bce", WALK_DIST, "spike_tile2", "walk, RotatE bce", directions=("sp",)),
]
SEED0 = 4300

# ---- the f32 family: (d, E, n, ent_ld), the SHAPES and WALK of tests/test_gpu_ce_f32.py --------------------------------
F_RAG, F_FULL, F_ONE, F_LD, F_BIG = (16, 150, 37, 16), (64, 128, 128, 64), (8, 129, 1, 8), (40, 128 * 17 + 1, 130, 48), \
    (128, 1037, 203, 128)
WALK_F32 = (8, 128 * 300 + 1, 130, 8)  # 301 tiles, col_tiles 2, 151 groups, the last one tile with one valid column
TARGET = {"ascending": 40.0, "descending": 40.0, "plateau": 112.0}  # (spikes: 128)


def _f3(name, kind, shape, profile, why, **kw):
    d, E, n, ld = shape
    return dict(name=name, l_norm=1.0, kind=kind, d=d, E=E, n=n, ent_ld=ld, profile=profile, why=why, **kw)


CASES_F32 = [
    _f3("complex", "ce", F_RAG, "ascending", "a second tile with 22 valid columns: the max rises in every 16-column step"),
    _f3("distmult", "kl", F_RAG, "spike_last", "the spike in the ragged tile; its second thread sees only padding"),
    _f3("complex", "bce", F_FULL, "descending", "exactly one full tile", g_scalar=-0.5),
    _f3("distmult", "klwb", F_FULL, "plateau", "weighted kl with label_bias, ties"),
    _f3("complex", "ce", F_ONE, "spike_last", "one row; the second tile has ONE valid column"),
    _f3("distmult", "kl", F_ONE, "spike_first", "one row, every entity a label", g_scalar=1.5),
    _f3("complex", "klwb", F_LD, "spike_last", "ent_ld 48 > d 40, 18 groups of one tile, the last with one valid column"),
    _f3("distmult", "ce", F_LD, "ascending", "ent_ld > d; K tail inside a chunk", g_scalar=0.25),
    _f3("complex", "kl", F_BIG, "descending", "four K chunks, two row tiles"),
    _f3("distmult", "ce", F_BIG, "spike_first", "|score| >= 100 at column 0"),
    _f3("complex", "bce", F_BIG, "plateau", "bce with an offset over 9 tiles"),
    _f3("complex", "ce", WALK_F32, "spike_tile2", "walk: the maximum arrives in the second walked tile", directions=("sp",)),
    _f3("distmult", "kl", WALK_F32, "ascending", "walk: the max rises in every step of every tile", directions=("po",)),
    _f3("complex", "bce", WALK_F32, "descending", "walk: the bce record summed across walked tiles", directions=("po",)),
    _f3("distmult", "ce", WALK_F32, "ascending", "walk, DistMult ce", directions=("sp",)),
    _f3("complex", "klwb", WALK_F32, "spike_last", "walk: the maximum in the short last group", directions=("po",)),
    _f3("distmult", "bce", WALK_F32, "spike_tile2", "walk, DistMult bce", directions=("sp",)),
]
SEED1 = 8300


def make_case_f32(c, direction="sp", seed=None):
    """Entity row j = pr_j amp w + noise, w = +-1/4 per coordinate (ComplEx: the real half) and the noise orthogonal to w;
    relation 0 is exactly 1 (+ 0 i), so a hot row (a = hot column, p = 0) has q = its entity row and scores
    TARGET pr_j + O(noise^2): the profile.  pr is constant over 16-column blocks (ascending / descending), so that the
    running max moves at every fold step.  The other rows take random entity and relation rows."""
    name, n, E, d, prof = c["name"], c["n"], c["E"], c["d"], c["profile"]
    if seed is None:
        seed = SEED1 + 100 * CASES_F32.index(c) + (0 if direction == "sp" else 1)
    rng = np.random.default_rng(seed)
    hot, walk = hot_columns(c), is_walk(c)
    j = np.arange(E)
    nblk = -(-E // 16)
    if prof in ("ascending", "descending"):
        pos = j // 16 if prof == "ascending" else nblk - 1 - j // 16
        pr = 0.05 + 0.95 * pos / max(nblk - 1, 1)
    else:
        pr = np.zeros(E)
        pr[hot] = 1.0
    h = d // 2 if name == "complex" else d
    w = np.zeros(d)
    w[:h] = rng.choice([-0.25, 0.25], h)
    amp = np.sqrt(TARGET.get(prof, 128.0) / (w @ w))
    noise = rng.standard_normal((E, d)) * 2.0 ** -6
    noise -= np.outer(noise @ w / (w @ w), w)
    ent = pr[:, None] * amp * w[None, :] + noise
    ent[hot] = ent[hot[0]]  # (plateau: identical rows)
    R_ = 5
    rel = rng.standard_normal((R_, d)) * 2.0 ** -7
    rel[:, :h] += 1.0
    rel[0] = 0.0
    rel[0, :h] = 1.0
    ent, rel = ent.astype(np.float32), rel.astype(np.float32)
    return _queries_and_labels(c, direction, rng, ent, rel, hot, int(hot[0]), walk, 3.0 - TARGET.get(prof, 128.0), R_)


def case_id(c):
    if c["name"] in F32:
        return f"{c['kind']}-{c['name']}-n{c['n']}-E{c['E']}-d{c['d']}-{c['profile']}"
    return f"{c['kind']}-{c['name']}-L{c['l_norm']:g}-n{c['n']}-E{c['E']}-d{c['d']}-{c['profile']}"


def directions(c):
    return c.get("directions", ("sp", "po"))


def is_walk(c):
    return groups(c["name"], c["n"], c["E"])[0] > 1


def walk_label_cols(n, m, name="transe"):
    """ce labels of a walked table: the later tiles of the first, of a middle and of the last full group, and the short
    last group"""
    T, G = groups(name, n, m)
    tw = geometry(name)[0]
    cols = [(g * T + t) * tw + 5 + t for g in (0, G // 2, G - 2) for t in range(1, T)]
    return cols + [m - 1]


def hot_columns(c):
    m, prof = c["E"], c["profile"]
    if prof in ("ascending", "spike_last"):
        return np.array([m - 1])
    if prof in ("descending", "spike_first"):
        return np.array([0])
    if prof == "spike_tile2":
        return np.array([geometry(c["name"])[0] + 37])
    if prof == "plateau":
        return np.arange(m - 7, m - 2)
    return np.array([PT + 5 if m > 2 * PT else 5])  # zero: the query's own row


def norm_factor(c):
    k = c["d"] if c["name"] == "transe" else c["d"] // 2
    return float(k) if c["l_norm"] == 1.0 else math.sqrt(k)


CASES = CASES_DIST + CASES_F32


def make_case(c, direction="sp", seed=None):
    """the inputs of one case of CASES_DIST or CASES_F32 and one direction"""
    return (make_case_f32 if c["name"] in F32 else make_case_dist)(c, direction, seed)


def make_case_dist(c, direction="sp", seed=None):
    """The inputs of one distance case and direction.  Entity row j lies at per-coordinate offset delta_j from the hot query Q0
    along a fixed direction, so that the hot rows (0, 8, 16, ..: a = a_hot, p = 0) score -nf delta_j up to the noise: the
    case's profile.  The other rows gather random entity and relation rows: scores of no particular shape."""
    name, lp, n, E, d, kind, prof = c["name"], c["l_norm"], c["n"], c["E"], c["d"], c["kind"], c["profile"]
    if seed is None:
        seed = SEED0 + 100 * CASES_DIST.index(c) + (0 if direction == "sp" else 1)
    rng = np.random.default_rng(seed)
    nf, hot, walk = norm_factor(c), hot_columns(c), cd_groups(n, E)[0] > 1
    j = np.arange(E)
    tiles = -(-E // PT)
    # ---- the distance profile D_j of the hot rows, as per-coordinate offsets
    mono = prof in ("ascending", "descending")
    if mono:  # whole grid steps per tile (TransE: delta stays on the grid), the within-tile variation below one step
        pos = (tiles - 1 - j // PT) if prof == "ascending" else j // PT
        step = max(1, int(round(SPAN / nf * GRID / max(tiles - 1, 1)))) if not walk else 1
        delta = np.ceil(BASE / nf * GRID) / GRID + pos * step / GRID
    elif prof == "zero":
        delta = (2.0 + 10.0 * rng.uniform(0, 1, E)) / nf
        delta[hot] = 0.0
    else:
        delta = np.full(E, (BASE + FAR) / nf) + rng.uniform(0, 4, E) / nf
        delta[hot] = BASE / nf
    # (the four 16-column slots of a tile on different levels too, so that the lane merge rescales)
    slot = np.zeros(E, np.int64)
    if mono:  # (walked: the short last group's single column sits in slot 0, which stays the closest)
        slot = 8 * ((3 - j // 16 % 4) if prof == "ascending" and not walk else j // 16 % 4)
    a_hot = {"ascending": 0, "descending": E - 1, "zero": int(hot[0])}.get(prof, E // 2)
    if prof != "zero":
        delta[a_hot] = delta.max() + 4.0 / nf  # the query's own row: the farthest target
    R_ = 5
    if name == "transe":
        delta = np.round(delta * GRID) / GRID
        s = rng.choice([-1.0, 1.0], d)
        Q0 = rng.integers(-128, 129, d) / GRID
        ent = Q0[None, :] + delta[:, None] * s[None, :]
        if walk or mono:
            ent[:, 0] += (j % 8 + slot) / GRID * s[0]
        elif prof != "plateau":
            ent += rng.integers(-1, 2, (E, d)) / GRID
        ent[hot] = Q0 + delta[hot][:, None] * s  # the hot columns: no noise (plateau: identical rows; zero: t = q)
        ent[a_hot] = Q0 + delta[a_hot] * s
        rel = rng.integers(-128, 129, (R_, d)) / GRID
        rel[0] = (Q0 - ent[a_hot]) if direction == "sp" else (ent[a_hot] - Q0)  # q = a + r (sp), a - r (po) = Q0 exactly
    else:
        h = d // 2
        M = max(1.0, float(delta.max()) / 2 + 0.5)
        th = rng.uniform(-np.pi, np.pi, h)
        Q0 = M * np.exp(1j * th)
        rad = delta[:, None] + ((j % 8 + slot)[:, None] / 32.0 * 0.5 / GRID if walk or mono else rng.uniform(0, 1, (E, h)) / GRID)
        ent_c = Q0[None, :] * (1 + rad / M)
        ent_c[hot] = Q0[None, :] * (1 + delta[hot][:, None] / M)
        phase0 = 0.0 if prof == "zero" else float(np.float32(np.pi))
        ent_c[a_hot] = Q0 * np.exp(-1j * phase0) if direction == "sp" else Q0 * np.exp(1j * phase0)
        ent = np.hstack([ent_c.real, ent_c.imag])
        rel = rng.uniform(0.1, np.pi - 0.1, (R_, h)) * rng.choice([-1.0, 1.0], (R_, h))
        rel[0] = phase0
    ent, rel = ent.astype(np.float32), rel.astype(np.float32)
    if name == "transe":
        assert np.array_equal(ent * GRID, np.round(ent * GRID)) and np.abs(ent).max() < 2.0 ** 10
    return _queries_and_labels(c, direction, rng, ent, rel, hot, a_hot, walk, 103.0 if prof != "zero" else 3.0, R_)


def _queries_and_labels(c, direction, rng, ent, rel, hot, a_hot, walk, offset, R_):
    """the query rows, upstream gradients and labels of a case (both families): hot rows 0, 8, 16, .. gather (a_hot, 0)"""
    name, n, E, kind, prof = c["name"], c["n"], c["E"], c["kind"], c["profile"]
    hot_rows = np.arange(0, n, 8)[:16]
    a = rng.integers(0, E, n)
    p = rng.integers(1, R_, n)
    a[hot_rows], p[hot_rows] = a_hot, 0
    out = dict(c)
    out.update(direction=direction, ent=ent, rel=rel, a=a.astype(np.int64), p=p.astype(np.int64), m=E, hot=hot,
               hot_rows=hot_rows, a_hot=a_hot, g_scalar=1.0, g_rows=None)
    gvals = np.array([1.0, 0.0, -0.5, 2.0 ** -10, 2.0 ** 10, 0.37, 1.5, 2.0 ** -3], np.float32)
    if c.get("g_scalar") is not None:
        out["g_scalar"] = float(c["g_scalar"])
    else:
        i = np.arange(n)
        out["g_rows"] = gvals[(i + i // 8) % gvals.size].copy()  # (the hot rows 0, 8, 16, .. take every value in turn)
        if n > 2:
            out["g_rows"][hot_rows[:2]] = (1.0, 0.37)  # the first two hot rows (label on / off the spike): not zero
    far = int((hot[0] + E // 2) % E)
    if kind == "ce":
        cols = [x for x in LABEL_COLS + (E - 1,) if x < E] + (walk_label_cols(n, E, name) if walk else [])
        lab = np.array(cols)[(np.arange(n) + np.arange(n) // 8) % len(cols)]
        lab[hot_rows[0::2]] = hot[0]   # the label on the spike: loss near 0, p - g cancels
        lab[hot_rows[1::2]] = far      # far from it
        if n == 1:
            lab[0] = geometry(name)[0] - 1  # far from the spike, and the last column of a chunk of the smallest width
        out["label"] = lab.astype(np.int64)
    else:
        edge = sorted({x for x in (0, 31, 32, 63, 64, 127, 128, E - 1) if x < E})
        rows = []
        for i in range(n):
            t = i % 8 if n > 4 else 4
            if i in hot_rows and n > 4:
                js = [int(hot[0])] if (i // 8) % 2 == 0 else [far, (far + 1) % E]
            elif t == 1:
                js = []
            elif t == 2:
                js = [edge[i // 8 % len(edge)]]
            elif t == 3:  # 65 labels (every entity of a smaller table): the second 64-entry pass of the finish kernel
                rest = [x for x in rng.permutation(E) if x not in edge]
                js = edge + rest[:max(0, min(65, E) - len(edge))]
            elif t == 4 and (E <= 150 or i == 4):
                js = list(range(E))  # every entity
            else:
                js = list(rng.choice(E, int(rng.integers(2, 9)), replace=False))
            rows.append(rng.permutation(np.asarray(js, np.int64)))
        out["rowptr"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        out["col"] = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
    if kind in ("klw", "klwb"):
        k_i = np.maximum(np.diff(out["rowptr"]), 1)
        out["kind"] = "kl"
        out["label_weight"] = (0.9 / k_i + rng.uniform(0, 0.01, n)).astype(np.float32)
    if kind == "klwb":  # label smoothing's uniform term (f32 family only: the scores are linear in the target)
        out["label_bias"] = np.full(n, 0.1 / E, np.float32)
    if kind == "bce":
        out["offset"] = offset  # |score + offset| of the hot spike: order 1
    # pairs at distance exactly zero (q == t in every coordinate)
    zp = np.zeros((n, E), bool)
    if prof == "zero":
        zp[hot_rows, hot[0]] = True
    out["zero_pairs"] = zp
    return out


def ref_lse32(x):
    """the float32 lse vector the backward is given: the float64 reference's, rounded (both test files use it)"""
    return lse64(x).astype(np.float32)


def oracle_scores(k):
    """the canonical float32 score bits [n, E] (oracle.score_sp / score_po: what kge_score_sp / kge_score_po store)"""
    import oracle as ko
    O = ko.Tables(k["name"], k["ent"], k["rel"], k["l_norm"])
    return ko.score_sp(O, k["a"], k["p"]) if k["direction"] == "sp" else ko.score_po(O, k["p"], k["a"])
