"""The fused bf16 ComplEx / DistMult losses (kge_ce_fwd/bwd, kge_ce_sp_po_fwd/bwd, kge_kl_fwd/bwd, kge_kl_weighted_fwd/bwd,
kge_bce_fwd/bwd: ce_loss.hip) restated in numpy float64 for the tests (no torch, no GPU), with elementwise bounds.  The
operand roundings (`bf16_rne`, `q16`), the gradient closed forms, `U` and `C_ACC` are those of _pairs_bwd16_ref.py.

SCORES      x64 = Q16 @ T^T in float64 from the bf16-valued tables (Q16 = RNE_bf16(fl32(a r)), the fragments of all three
            kernel generations).  B_x = C_ACC d u (|Q16| @ |T|^T): d exact products accumulated in float32 on the matrix
            core.  As in _pairs_bwd16_ref, C_ACC = 2 is AN ASSUMPTION about the additions inside
            v_mfma_f32_32x32x16_bf16, not a measurement.

ASSUMPTION ABOUT THE TRANSCENDENTAL INSTRUCTIONS.  C_TR = 2 (units of u = 2^-24, i.e. 1 ulp): the CDNA ISA documentation
            lists V_EXP_F32 and V_LOG_F32 at 1 ULP; libm's expf / logf (ce_combine_kernel) are documented at 1 ulp too.
            v_exp_f32 does not produce denormals: a result below 2^-126 may come out as zero (FLUSH).  These are read off
            the documentation, never tuned to the kernel's output: a ratio above 1 in tests/test_gpu_ce16_bound.py is a
            finding about a kernel or about C_TR / C_ACC, told apart by forcing the other kernel generation.
            Float32 division (V3_DSIG, kl_sub_kernel's g / k) is correctly rounded (the library is built without fast
            math; hipcc's default for float division).

FORWARD     lse given the score bits x of a row (X = max |x|, rng = max x - min x, m columns, S = ceil(m / 32) sub-units;
            every sum below is a sum of positive terms, so a term's relative error is bounded by the roundings on ITS
            path).  rho = relative error of L = sum_j exp(x_j - M), in units of u:
              3 X        V3_LOG2E rounded (x c: u |x|, ce_pairs_v8.hip:214) + n2 = fl(mx c) (:211) and pp[0] = M2 * V3_LN2
                         with V3_LN2 rounded (:302): 2 u |mx| (v4 / v3 store the max itself: less)
              2 rng      the exponent of a term: fma(x, c, -n2) one rounding u |t| (v8 :214); (x - rf) * c two roundings
                         (score_pairs_bf16_v4.hip:753, score_pairs_bf16_v3.hip:504/603): 2 u |x - rf| in nats
              C_TR       exp2 of the term
              32         additions of the terms of one tile in a lane (16 per sub-unit in v8 :214, 32 per tile in v4 :753
                         and v3 :504-507): a term passes at most that many
              (S + 2)(C_TR + 2)   one rescale per later sub-unit (rsum * 2^(m2 - n2) + sm: exp2, product, sum; v8 :215,
                         v4 :754, v3 :510/605) and the merge of the two lanes of a row (v8 :295, v4 :878, v3 :611)
              2 rng      the exponents of the rescales telescope to at most the range (subtraction and, v4 / v3, the
                         product by V3_LOG2E)
              C_TR + 2 + rng   ce_combine_kernel :93 (kl_*_combine :247/:282): expf(p_c - M), its argument's subtraction
                         (u |p_c - M| <= u rng), the product
              ceil(S / 64) + 7     the sum over the column groups (at most S of them): lane loop + six butterfly steps
            b_lse = rho (1 + rho) + C_TR u log m  [logf(L), L in [1, m]]  + u (X + log m)  [z = M + logf(L) :97]
                    + FLUSH: 2 m (S + 1) 2^-126 (every term and every rescale factor below 2^-126 may read zero)
            ce    loss = z - x[label] (:100): b_lse + u |loss|
            kl    label scores by kl_label_sum (ce_loss.hip:183-208): exact products, 8 fma + 6 butterfly additions
                  -> 14 u (|Q16| . |T_j|) each against x64; their sum in label order (k - 1) u sum |x|; / k, logf(k),
                  two subtractions (:257/:290).  Weighted: z - w * tsum (:256/:289): product and subtraction
            bce   v3_softplus (common.hpp:397-401) per term: u |x + off| (the addition) + (C_TR + 1) u (e = exp2(-|x| c):
                  e (C_TR + 2 |x|) u <= that) + max(2^-21 / 3 [series, e < 2^-7: e^3 / 3], (C_TR + 3) u [1 + e, v_log_f32,
                  * V3_LN2]) + u sp (the final addition); a term passes at most 32 + S + ceil(S / 64) + 7 + 1 additions
                  (score_pairs_bf16_v3.hip:519/628/632, bce_combine_kernel :334-336); label sums as for kl; k * offset,
                  the sum and the subtraction (:339)

GRADIENT COEFFICIENTS (G16).  kge_*_bwd takes lse as an input: the reference uses the same float32 vector.  From the
            score bits x, in float64, tau = (x - lse) log2(e) and p = g (2^tau - b) - g [j = label]; for bce
            p = g sigmoid(x + offset).  The kernel's float32 value before its bf16 rounding lies in [p - e, p + e]:
              exponent   |t - tau| <= u (3 |tau| + c |lse|) (1 + 2^-10): v8 (ce_pairs_v8.hip:231/:396) l2 = fl(lse c),
                         fma(x, c, -l2): u (|tau| [c] + c |lse| [l2] + |t| [fma]); v4 / v3 (score_pairs_bf16_v4.hip:721,
                         score_pairs_bf16_v3.hip:357) (x - lse) * c: 3 u |tau|.  The union covers every route, so forced
                         routes get the same interval.  2^-10 absorbs the second-order terms
              exp2       (1 +- C_TR u), or zero below 2^-126
              product    v8: fma(e, g, -gb) one rounding; v4 / v3: fl(fl(e g) - gb) two: u (|e g| + |v|), + 2^-149
              label      p - g: one more rounding u |p - g| + 2^-149 (v8 :236, v4 :724)
              bce        z = fl(x + off), w = fl(-z c): 3 u |tau|; 1 + e and g / den: one rounding each
            G_lo = bf16_rne(p - e), G_hi = bf16_rne(p + e), the float64 -> float32 step rounded OUTWARD (nextafter):
            rounding is monotone, so the kernel's G16 lies in [G_lo, G_hi]; an element is DECIDED where G_lo == G_hi.
            kl / bce: kl_sub_kernel / bce_sub_kernel (ce_loss.hip:295-315, :344-361) subtract y from the ALREADY ROUNDED
            G16 and round again -- two roundings, restated in that order in float32 (monotone in G16).
            Pad columns [m, ld16) are zero.

GRADIENTS   pairs_bwd16's closed forms on G_c = (G_lo + G_hi) / 2 with Q16; bound = the accumulation bound of
            pairs_bwd16_bound on max(|G_lo|, |G_hi|) plus the slack G_r^T |Q16| (g_tgt) / G_r |T| pushed through the
            chain (g_a, g_p), G_r = (G_hi - G_lo) / 2.  Two-sided entries stack the 2n rows as the library does.

The fixed case list (`CASES_CE`, `make_case`) and the host rule (`v8_takes`, `route`) are here so that the CPU file checks
the very inputs the GPU file runs.  The branch of every case is its `why`.
"""
import numpy as np

import _pairs_bwd_ref as R
import _pairs_bwd16_ref as R16
from _pairs_bwd16_ref import bf16_rne, q16, U, C_ACC  # noqa: F401  (pairs_bwd16's closed forms: R._dot)

C_TR = 2
LOG2E = 1.4426950408889634
LOG2E_F = np.float32(1.44269504088896340736)
LN2_F = np.float32(0.69314718055994530942)
TINY = 2.0 ** -126
SUB = 2.0 ** -149
F32MAX = float(np.finfo(np.float32).max)


# ---- scores ------------------------------------------------------------------------------------------------------------
def operands(k, side=None):
    """(Q16 [rows, d], T [m, d], A, Rr) in float64; two-sided cases: side 0 (sp, a = s), 1 (po, a = o) or None = stacked"""
    ent, rel = k["ent"], k["rel"]
    if k["kind"] == "ce2":
        if side is None:
            parts = [operands(k, 0), operands(k, 1)]
            return tuple(np.vstack([x[i] for x in parts]) if i != 1 else parts[0][1] for i in range(4))
        a, direction = (k["a"], "sp") if side == 0 else (k["o"], "po")
    else:
        a, direction = k["a"], k["direction"]
    A, Rr = ent[a], rel[k["p"]]
    Q = q16(k["name"], direction, A, Rr).astype(np.float64)
    return Q, ent.astype(np.float64), A.astype(np.float64), Rr.astype(np.float64)


def scores64(k):
    Q, T, _, _ = operands(k)
    return Q @ T.T


def score_bound(k):
    Q, T, _, _ = operands(k)
    return C_ACC * k["d"] * U * (np.abs(Q) @ np.abs(T).T)


# ---- forward -----------------------------------------------------------------------------------------------------------
def lse64(x):
    x = np.asarray(x, np.float64)
    mx = x.max(axis=1)
    return mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))


def lse_bound(x):
    """|kernel lse - lse64(x)| for the kernel's own score bits x (module docstring, FORWARD)"""
    x = np.asarray(x, np.float64)
    m = x.shape[1]
    S = -(-m // 32)
    X, rng = np.abs(x).max(axis=1), x.max(axis=1) - x.min(axis=1)
    rho = U * (3 * X + 5 * rng + C_TR + 32 + (S + 2) * (C_TR + 2) + (C_TR + 2) + (-(-S // 64) + 7))
    return rho * (1 + rho) + C_TR * U * np.log(m) + U * (X + np.log(m)) + 2 * m * (S + 1) * TINY


def labels_of(k, side=None):
    """index labels of the rows (ce / ce2), stacked for two-sided"""
    return np.concatenate([k["label"], k["label2"]]) if k["kind"] == "ce2" else k["label"]


def ce64(x, label):
    z = lse64(x)
    return z - np.asarray(x, np.float64)[np.arange(len(label)), label], z


def ce_bound(x, label):
    loss, _ = ce64(x, label)
    return lse_bound(x) + U * np.abs(loss)


def _csr_rows(k):
    rp, col = k["rowptr"], k["col"]
    return [col[rp[i]:rp[i + 1]] for i in range(len(rp) - 1)]


def kl64(x, k, x_label=None):
    """(loss_rows, lse): 1/k_i labels (rows without labels: 0), or lse - w_i sum (weighted); x_label: the scores the
    label terms are taken from (kl_label_sum evaluates them itself: not the matrix core's bits)"""
    z = lse64(x)
    x = np.asarray(x if x_label is None else x_label, np.float64)
    loss = np.zeros(len(x))
    for i, js in enumerate(_csr_rows(k)):
        if k.get("label_weight") is not None:
            loss[i] = z[i] - float(k["label_weight"][i]) * x[i, js].sum()
        elif len(js):
            loss[i] = z[i] - x[i, js].mean() - np.log(len(js))
    return loss, z


def _label_sum_bound(k, i, js, x):
    """kl_label_sum against the exact label scores: 14 roundings per score + the sum in label order"""
    Q, T, _, _ = operands(k)
    return 14 * U * (np.abs(Q[i]) @ np.abs(T[js]).T).sum() + max(len(js) - 1, 0) * U * np.abs(x[i, js]).sum()


def kl_bound(x, k, x_label=None):
    """bound of kl64's loss rows: lse from the bits x, the label scores against x_label (default x) by kl_label_sum"""
    x = np.asarray(x, np.float64)
    xl = x if x_label is None else np.asarray(x_label, np.float64)
    loss, z = kl64(x, k, xl)
    b = lse_bound(x)
    for i, js in enumerate(_csr_rows(k)):
        if len(js) == 0 and k.get("label_weight") is None:
            b[i] = 0.0
            continue
        s = _label_sum_bound(k, i, js, xl)
        t = np.abs(xl[i, js]).sum()
        if k.get("label_weight") is not None:
            w = abs(float(k["label_weight"][i]))
            b[i] += w * s + U * w * t + U * np.abs(loss[i])
        else:
            kk = len(js)
            b[i] += s / kk + U * t / kk + C_TR * U * np.log(kk) + U * (np.abs(z[i]) + t / kk) + U * np.abs(loss[i])
    return b


def bce64(x, k, x_label=None):
    xo = np.asarray(x, np.float64) + float(k["offset"])
    xl = xo if x_label is None else np.asarray(x_label, np.float64) + float(k["offset"])
    sp = np.maximum(xo, 0) + np.log1p(np.exp(-np.abs(xo)))
    loss = sp.sum(axis=1)
    for i, js in enumerate(_csr_rows(k)):
        loss[i] -= xl[i, js].sum()
    return loss


def bce_bound(x, k, x_label=None):
    x = np.asarray(x, np.float64)
    xl = x if x_label is None else np.asarray(x_label, np.float64)
    off = float(k["offset"])
    xo = x + off
    m = x.shape[1]
    S = -(-m // 64)
    sp = np.maximum(xo, 0) + np.log1p(np.exp(-np.abs(xo)))
    e = np.exp(-np.abs(xo))
    per = U * np.abs(xo) + (C_TR + 1) * U + np.where(e < 2.0 ** -7, 2.0 ** -21 / 3, (C_TR + 3) * U) + U * sp
    depth = 32 + S + (-(-S // 64) + 7) + 1
    b = per.sum(axis=1) + depth * U * sp.sum(axis=1)
    loss = bce64(x, k, xl)
    for i, js in enumerate(_csr_rows(k)):
        t = np.abs(xl[i, js]).sum() + len(js) * abs(off)
        b[i] += _label_sum_bound(k, i, js, xl) + 2 * U * t + U * np.abs(loss[i])
    return b


# ---- gradient coefficients ---------------------------------------------------------------------------------------------
def _out32(lo, hi):
    """float64 interval -> float32 ends rounded outward"""
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32, hi32


def row_gradients(k):
    """(g [rows] float32 as the kernel reads it, gb = fl(g bias) float32)"""
    rows = k["rows"]
    g = np.full(rows, np.float32(k["g_scalar"]), np.float32) if k.get("g_rows") is None else k["g_rows"].astype(np.float32)
    if k["kind"] == "kl" and k.get("label_weight") is None:  # rows without labels: zero gradient (ce.rowptr given; not under label_weight)
        cnt = np.diff(k["rowptr"])
        g = np.where(cnt == 0, np.float32(0), g)
    gb = np.zeros(rows, np.float32) if k.get("label_bias") is None else g * k["label_bias"].astype(np.float32)
    return g, gb


def _sub_y(k):
    """what kl_sub_kernel / bce_sub_kernel subtract at the labels of a row (float32, the kernels' expressions)"""
    rows = k["rows"]
    gi = np.full(rows, np.float32(k["g_scalar"]), np.float32) if k.get("g_rows") is None else k["g_rows"].astype(np.float32)
    if k["kind"] == "bce":
        return gi
    if k.get("label_weight") is not None:
        return gi * k["label_weight"].astype(np.float32)
    cnt = np.maximum(np.diff(k["rowptr"]), 1).astype(np.float32)
    return gi / cnt


def g16_interval(k, x, lse32=None):
    """-> (G_lo, G_hi) float32 arrays of bf16 values [rows, m] (module docstring, GRADIENT COEFFICIENTS)"""
    x = np.asarray(x, np.float64)
    rows, m = x.shape
    g32, gb32 = row_gradients(k)
    g, gb = g32.astype(np.float64)[:, None], gb32.astype(np.float64)[:, None]
    ag = np.abs(g)
    one = 1 + 2.0 ** -10
    if k["kind"] == "bce":
        tau = -(x + float(k["offset"])) * LOG2E
        dt = 3 * U * np.abs(tau) * one
        with np.errstate(over="ignore"):
            e_hi = np.exp2(np.minimum(tau + dt, 1000.0)) * (1 + C_TR * U)
            e_lo = np.exp2(tau - dt) * (1 - C_TR * U)
        e_lo = np.where(e_lo < TINY * one, 0.0, e_lo)
        den_lo, den_hi = (1 + e_lo) * (1 - U), (1 + e_hi) * (1 + U)
        mag_hi = ag / den_lo * (1 + U) + SUB
        mag_lo = np.where(den_hi >= F32MAX, 0.0, np.maximum(ag / den_hi * (1 - U) - SUB, 0.0))
        lo = np.where(g >= 0, mag_lo, -mag_hi)
        hi = np.where(g >= 0, mag_hi, -mag_lo)
    else:
        lse = np.asarray(lse32, np.float32).astype(np.float64)[:, None]
        tau = (x - lse) * LOG2E
        dt = U * (3 * np.abs(tau) + LOG2E * np.abs(lse)) * one
        e_hi = np.exp2(tau + dt) * (1 + C_TR * U)
        e_lo = np.exp2(tau - dt) * (1 - C_TR * U)
        e_lo = np.where(e_lo < TINY * one, 0.0, e_lo)
        v_lo = np.where(g >= 0, e_lo * g, e_hi * g) - gb
        v_hi = np.where(g >= 0, e_hi * g, e_lo * g) - gb
        r = U * (e_hi * ag + np.maximum(np.abs(v_lo), np.abs(v_hi))) * one + SUB
        lo, hi = v_lo - r, v_hi + r
        if k["kind"] in ("ce", "ce2"):
            lab = labels_of(k)
            i = np.arange(rows)
            l2, h2 = lo[i, lab] - g[:, 0], hi[i, lab] - g[:, 0]
            r2 = U * np.maximum(np.abs(l2), np.abs(h2)) * one + SUB
            lo[i, lab], hi[i, lab] = l2 - r2, h2 + r2
    lo32, hi32 = _out32(lo, hi)
    G_lo, G_hi = bf16_rne(lo32), bf16_rne(hi32)
    if k["kind"] in ("kl", "bce"):  # the second kernel: G16 - y, rounded again
        y = _sub_y(k)
        for i, js in enumerate(_csr_rows(k)):
            if len(js):
                G_lo[i, js] = bf16_rne(G_lo[i, js] - y[i])
                G_hi[i, js] = bf16_rne(G_hi[i, js] - y[i])
    return G_lo, G_hi


# ---- gradients ---------------------------------------------------------------------------------------------------------
def _sides(k):
    if k["kind"] == "ce2":
        n = k["n"]
        return [("sp", slice(0, n)), ("po", slice(n, 2 * n))]
    return [(k["direction"], slice(0, k["rows"]))]


def grads_from_g16(k, G, pad_one=False):
    """(g_a, g_p, g_tgt) in float64 from a coefficient matrix G [rows, m] and the rounded queries Q16"""
    G = np.asarray(G, np.float64)
    Q, T, A, Rr = operands(k)
    if pad_one:  # planted: the first pad column holds 1.0; the product multiplies it with the clamped last target row
        G, T2 = np.hstack([G, np.ones((G.shape[0], 1))]), np.vstack([T, T[-1:]])
    else:
        T2 = T
    ga, gp = np.zeros_like(A), np.zeros_like(A)
    for direction, sl in _sides(k):
        ga[sl], gp[sl], _ = R._dot(k["name"], direction, A[sl], Rr[sl], T2, G[sl], G[sl], -1.0)
    return ga, gp, G[:, :T.shape[0]].T @ Q


def grads_and_bound(k, G_lo, G_hi):
    """-> ((g_a, g_p, g_tgt), (b_a, b_p, b_tgt)) (module docstring, GRADIENTS)"""
    lo, hi = np.asarray(G_lo, np.float64), np.asarray(G_hi, np.float64)
    Gc, Gr, Gm = (lo + hi) / 2, (hi - lo) / 2, np.maximum(np.abs(lo), np.abs(hi))
    want = grads_from_g16(k, Gc)
    Q, T, A, Rr = operands(k)
    rows, m = Gc.shape
    cc = R16.C_CHAIN16[k["name"]]
    ba, bp = np.zeros_like(A), np.zeros_like(A)
    for direction, sl in _sides(k):
        ca, cp, _ = R._dot(k["name"], direction, np.abs(A[sl]), np.abs(Rr[sl]), np.abs(T), Gm[sl], Gm[sl], 1.0)
        sa, sp_, _ = R._dot(k["name"], direction, np.abs(A[sl]), np.abs(Rr[sl]), np.abs(T), Gr[sl], Gr[sl], 1.0)
        ba[sl], bp[sl] = (C_ACC * m + cc) * U * ca + sa * (1 + cc * U), (C_ACC * m + cc) * U * cp + sp_ * (1 + cc * U)
    bt = (C_ACC * rows + R16.C_TGT16) * U * (Gm.T @ np.abs(Q)) + Gr.T @ np.abs(Q)
    return want, (ba, bp, bt)


# ---- float32 restatement of the epilogue arithmetic (numpy; exp2 correctly rounded, inside C_TR) ------------------------
def _exp2f(t32):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(t32.astype(np.float64)).astype(np.float32)


def g16_restated(k, x32, lse32, form, defect=None):
    """G16 [rows, m] (bf16 values as float32) by the float32 arithmetic of one kernel generation: form 'v8'
    (ce_pairs_v8.hip ds_sub) or 'v4' (score_pairs_bf16_v4.hip ds_tile = score_pairs_bf16_v3.hip).  `defect`:
      label_plus4   the label subtracted at column label + 4 (the other lane of the row)
      label_last    the subtraction skipped where the label lies in the table's last 32-column sub-unit
      g_next        g_i taken from row i + 1
      drop_row      the last row of the first 256-row chunk written as zeros
      trunc         G16 truncated instead of rounded to nearest even
      sub_before    kl / bce: the label term subtracted before the rounding (one rounding instead of two)
      no_offset     bce: the offset ignored"""
    defect = defect or {}
    x = np.asarray(x32, np.float32)
    rows, m = x.shape
    g, gb = row_gradients(k)
    if defect.get("g_next"):
        g, gb = np.roll(g, -1), np.roll(gb, -1)
    g, gb = g[:, None], gb[:, None]
    rnd = R16.bf16_trunc if defect.get("trunc") else bf16_rne
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if k["kind"] == "bce":
            off = np.float32(0.0 if defect.get("no_offset") else k["offset"])
            p = g / (np.float32(1) + _exp2f(-(x + off) * LOG2E_F))
        elif form == "v8":
            l2 = (np.asarray(lse32, np.float32) * LOG2E_F)[:, None]
            t = (x.astype(np.float64) * np.float64(LOG2E_F) - l2).astype(np.float32)  # fma: one rounding
            p = (_exp2f(t).astype(np.float64) * g - gb).astype(np.float32)
        else:
            p = _exp2f((x - np.asarray(lse32, np.float32)[:, None]) * LOG2E_F) * g - gb
    i = np.arange(rows)
    if k["kind"] in ("ce", "ce2"):
        lab = labels_of(k).copy()
        do = np.ones(rows, bool)
        if defect.get("label_last"):
            do &= lab < (m - 1) // 32 * 32
        if defect.get("label_plus4"):
            lab = lab + 4
            do &= lab < m
        p[i[do], lab[do]] = p[i[do], lab[do]] - g[do, 0]
    y = _sub_y(k) if k["kind"] in ("kl", "bce") else None
    if y is not None and defect.get("sub_before"):
        for r_, js in enumerate(_csr_rows(k)):
            p[r_, js] = p[r_, js] - y[r_]
    G = rnd(p)
    if y is not None and not defect.get("sub_before"):
        for r_, js in enumerate(_csr_rows(k)):
            if len(js):
                G[r_, js] = rnd(G[r_, js] - y[r_])
    if defect.get("drop_row"):
        G[min(255, rows - 1)] = 0.0
    return G


def lse_restated(x32, defect=None):
    """float32 lse [rows] by the online softmax of ce_pairs_v8.hip lse_sub over 32-column sub-units (one column group, the
    two lanes of a row folded into one) + ce_combine_kernel.  `defect`:
      no_rescale    the factor 2^(m2 - n2) dropped when the max rises
      no_mask       the ragged last sub-unit unmasked: its pad columns count as score 0"""
    defect = defect or {}
    x = np.asarray(x32, np.float32)
    rows, m = x.shape
    S = -(-m // 32)
    xp = np.full((rows, S * 32), np.float32(0.0 if defect.get("no_mask") else -np.inf), np.float32)
    xp[:, :m] = x
    rmax = np.full(rows, -np.inf, np.float32)
    m2 = np.full(rows, -np.inf, np.float32)
    rsum = np.zeros(rows, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for s in range(S):
            v = xp[:, 32 * s:32 * s + 32]
            mx = np.maximum(rmax, v.max(axis=1))
            n2 = np.where(np.isinf(mx), np.float32(0), mx * LOG2E_F)
            t = (v.astype(np.float64) * np.float64(LOG2E_F) - n2[:, None]).astype(np.float32)
            sm = np.zeros(rows, np.float32)
            for c in range(32):
                sm = sm + _exp2f(t[:, c])
            f = np.float32(1) if defect.get("no_rescale") else _exp2f(m2 - n2)
            rsum = (rsum.astype(np.float64) * np.asarray(f, np.float64) + sm).astype(np.float32) if s else sm
            m2, rmax = mx * LOG2E_F, mx
        M = m2 * LN2_F
        return M + np.log(rsum.astype(np.float64)).astype(np.float32)


# ---- the host rule -----------------------------------------------------------------------------------------------------
def v8_takes(d, n, m):
    """pairs_bf16_v8_ce_takes (ce_pairs_v8.hip)"""
    tail = n % 256
    return d in (256, 512) and n > 128 and (tail == 0 or tail > 128 or n >= 1024) and m >= 1


def route(case, epi):
    """the kernel generation one pass of a case runs on: ce_takes_v8 / run_ds_pass / run_lse_pass / run_bce_fwd
    (ce_loss.hip).  epi: 'lse', 'ds', 'dsig', 'splus'."""
    d, n, m, sw = case["d"], case["n"], case["E"], case.get("switch") or {}
    if epi == "splus" or d == 128 or sw.get("CE_V3") == 1:
        return "v3"
    if epi in ("lse", "ds"):
        e = sw.get("CE_V8")
        if e == 1 or (e is None and v8_takes(d, n, m)):
            return "v8"
    return "v4"


# ---- the fixed cases ---------------------------------------------------------------------------------------------------
LABEL_COLS = (0, 3, 4, 7, 8, 31, 32, 63, 64)


def _c(name, kind, n, E, d, profile, why, **kw):
    return dict(name=name, kind=kind, n=n, E=E, d=d, profile=profile, why=why, **kw)


CASES_CE = [
    _c("complex", "ce", 1, 33, 128, "spike_last", "v3 (d = 128), one row, one ragged unit"),
    _c("distmult", "ce", 129, 65, 128, "ascending", "v3 (d = 128), two row groups"),
    _c("complex", "ce", 128, 64, 256, "descending", "v4 (n <= 128), exactly one tile"),
    _c("distmult", "ce", 300, 1037, 512, "ascending", "v4 (n = 300: tail 44 fails pairs_bf16_v8_ce_takes)", g_scalar=0.25),
    _c("complex", "ce", 129, 1037, 512, "ascending", "v8 by default (tail 129 > 128), 33 units: most XCD slices empty"),
    _c("distmult", "ce", 256, 2053, 256, "spike_first", "v8 by default (tail 0), d = 256: two sub-units per unit, every XCD slice"),
    _c("complex", "ce", 257, 65, 256, "plateau", "v4 (tail 1); forced v8 below"),
    _c("complex", "ce", 257, 65, 256, "plateau", "v8 forced (CE_V8 = 1) on the shape above", switch={"CE_V8": 1}),
    _c("distmult", "ce", 256, 2053, 256, "spike_first", "v4 forced (CE_V8 = 0) on a default-v8 shape", switch={"CE_V8": 0}),
    _c("complex", "ce", 129, 1037, 512, "ascending", "v3 forced (CE_V3 = 1) at d = 512", switch={"CE_V3": 1}),
    _c("distmult", "ce2", 513, 33, 512, "spike_last", "two-sided, v4 (tail 1), one ragged unit"),
    _c("complex", "ce2", 256, 1037, 256, "descending", "two-sided, v8"),
    _c("complex", "kl", 129, 1037, 256, "ascending", "kl, v8 gradient pass + kl_sub_kernel"),
    _c("distmult", "klw", 128, 65, 512, "plateau", "weighted kl with label_bias, v4"),
    _c("complex", "bce", 129, 1037, 256, "ascending", "bce: softplus on v3, sigmoid on v4"),
    _c("distmult", "bce", 37, 65, 128, "spike_first", "bce: softplus and sigmoid on v3 (d = 128)"),
]

TARGET = {"ascending": 40.0, "descending": 40.0, "spike_first": 128.0, "spike_last": 128.0, "plateau": 112.0}
SEED0 = 5100  # (seeds were tried on the CPU until the reference alone met the conditions of tests/test_ce16_ref_cpu.py)


def case_id(c):
    sw = "".join(f"-{a}{b}" for a, b in (c.get("switch") or {}).items())
    return f"{c['kind']}-{c['name']}-n{c['n']}-E{c['E']}-d{c['d']}-{c['profile']}{sw}"


def profile(c):
    """the column profile in [0, 1] and the hot column(s)"""
    m, kind = c["E"], c["profile"]
    if kind == "ascending":
        return np.linspace(0.05, 1.0, m), np.array([m - 1])
    if kind == "descending":
        return np.linspace(1.0, 0.05, m), np.array([0])
    pr = np.zeros(m)
    hot = {"spike_first": np.array([0]), "spike_last": np.array([m - 1]),
           "plateau": np.arange(m - 7, m - 2) if m > 40 else np.array([m - 1])}[kind]
    pr[hot] = 1.0
    return pr, hot


def make_case(c, direction="sp", seed=None):
    """The inputs of one case (and direction, for the one-sided kinds); `rows` = n, or 2n stacked for ce2.
    Entity row j = c_j w + noise (bf16-exact), w = +-1/4 per coordinate; a hot query row takes the hot entity, so that its
    score row is TARGET * profile (max |score| >= 100 for spikes and plateaus); the other rows take low-profile entities
    (scores of order 1).  Relation rows are 1 + noise (ComplEx: imaginary part noise)."""
    name, n, E, d, kind = c["name"], c["n"], c["E"], c["d"], c["kind"]
    if seed is None:
        seed = SEED0 + 100 * CASES_CE.index(c) + (0 if direction == "sp" else 1)
    rng = np.random.default_rng(seed)
    pr, hot = profile(c)
    h = d // 2 if name == "complex" else d
    w = np.zeros(d)
    w[:h] = rng.choice([-0.25, 0.25], h)  # ComplEx: w real, so q = a r keeps the alignment in both directions
    amp = np.sqrt(TARGET[c["profile"]] / (w @ w))
    ent = pr[:, None] * amp * w[None, :] + rng.standard_normal((E, d)) * 2.0 ** -6
    if c["profile"] == "plateau":
        ent[hot] = ent[hot[0]]  # identical rows: exact ties at the max
    ent = bf16_rne(ent.astype(np.float32))
    nrel = 5
    rel = rng.standard_normal((nrel, d)) * 2.0 ** -7
    rel[:, :h] += 1.0
    rel = bf16_rne(rel.astype(np.float32))
    cold = np.flatnonzero(pr <= 0.15)
    cold = cold if cold.size else np.arange(E)

    def queries(nn):
        a = rng.choice(cold, nn)
        hot_rows = np.arange(0, nn, 8)[:16]
        a[hot_rows] = hot[0]
        return a, hot_rows

    def labels(nn, hot_rows):
        cols = np.array([j for j in LABEL_COLS + (E - 1, (E - 1) // 32 * 32) if j < E])
        lab = cols[np.arange(nn) % cols.size]
        lab[hot_rows[0::2]] = hot[0]                      # the label on the spike: loss near 0, p - g cancels
        lab[hot_rows[1::2]] = (hot[0] + E // 2) % E       # far from it: softmax below float32's smallest normal
        if nn == 1:  # (a lone row: far -- the cancelling element would be 1 undecided of m, above any small share)
            lab[0] = (hot[0] + E // 2) % E
        return lab

    a, hot_rows = queries(n)
    p = rng.integers(0, nrel, n)
    rows = 2 * n if kind == "ce2" else n
    out = dict(c)
    out.update(direction=direction, ent=ent, rel=rel, a=a.astype(np.int64), p=p.astype(np.int64), rows=rows, m=E,
               hot_rows=hot_rows, hot=hot, g_scalar=1.0, g_rows=None)
    gvals = np.array([1.0, 0.0, -0.5, 2.0 ** -10, 2.0 ** 10, 0.37, 1.5, 2.0 ** -3], np.float32)
    if c.get("g_scalar") is not None:
        out["g_scalar"] = float(c["g_scalar"])
    else:
        i = np.arange(rows)
        out["g_rows"] = gvals[(i + i // 8) % gvals.size].copy()  # (the hot rows 0, 8, 16, .. take every value in turn)
    if kind in ("ce", "ce2"):
        out["label"] = labels(n, hot_rows).astype(np.int64)
    if kind == "ce2":
        # kge_ce_sp_po_*: the sp_ rows' labels are the objects, the _po rows' labels the subjects; the objects sit on the
        # listed columns (on / far from the spike for the hot rows) and are the query entities of the second side
        out["o"] = out["label"]
        out["label2"] = out["a"]
    if kind in ("kl", "klw", "bce"):
        cnts = np.array([0, 1, min(E, 40), 2, 3])[np.arange(n) % 5]
        cols = []
        for i, cn in enumerate(cnts):
            js = rng.choice(E, cn, replace=False)
            if cn >= 2:
                js[0], js[1] = 0, E - 1  # labels at the first and the last column
                js = np.unique(js)
                cnts[i] = js.size
            elif cn == 1:
                js[0] = (0, E - 1, hot[0])[i % 3]
            cols.append(np.sort(js))
        out["rowptr"] = np.concatenate([[0], np.cumsum(cnts)]).astype(np.int64)
        out["col"] = np.concatenate(cols + [np.zeros(0, np.int64)]).astype(np.int64)
    if kind == "klw":
        k_i = np.maximum(np.diff(out["rowptr"]), 1)
        out["kind"] = "kl"
        out["label_weight"] = (0.9 / k_i + rng.uniform(0, 0.01, n)).astype(np.float32)
        out["label_bias"] = np.full(n, 0.1 / E, np.float32)
    if kind == "bce":
        out["offset"] = -1.5
    return out


def ref_lse32(k, x=None):
    """the float32 lse vector the backward is given: the float64 reference's, rounded (both test files use it)"""
    return lse64(scores64(k) if x is None else x).astype(np.float32)


def directions(c):
    return ("sp",) if c["kind"] == "ce2" else ("sp", "po")
