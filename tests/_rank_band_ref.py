"""Float64 reference of the parity-mode ranking counts (split queries, band-and-rescore) -- CPU only.

What the kernels compute, per query row i and table row j of a slice:

    x_hi = fl32-chain(sum_k q_hi[i,k] t[j,k]),  x_lo = fl32-chain(sum_k q_lo[i,k] t[j,k]),  x = fl32(x_hi + x_lo)
    close = (x == t_i) | (isfinite(|x - t_i|) & (fl32(x - t_i) in [-allowed_i, allowed_i])),
    allowed_i = fl32(atol + |fl32(rtol t_i)|),   ties += close,   rank += (x > t_i) & !close

with NaN scores (and a NaN true score) taken as -inf and filtered columns (except the row's own target) as -inf
(include/kge_amd.h: kge_rank_counts).  q_hi = bf16(fl32(q)), q_lo = bf16(fl32(q) - q_hi) (bf16_queries.hpp), every
product q t of two bf16 values is exact in float32.  The band launch decides a pair from x_hi alone whenever
|x_hi - t_i| lies outside allowed_i + band_i, band_i >= |x_lo| by Cauchy-Schwarz: band_i ~ ||q_lo_i|| max_j ||t_j||.

The reference holds everything in float64 (bf16 values, their products and their squares are exact there) and carries
a DERIVED bound e_ij on |x_kernel - x64| (`margin64`): a column whose float64 score lies within e_ij of an edge of the
tie band is "undecided" and widens the interval of counts instead of being guessed.

Nothing here is fitted to a kernel's output; u = 2^-24 is the unit roundoff of float32 throughout."""
import fractions
import types

import numpy as np
import torch

U = 2.0 ** -24
GREATER, CLOSE, SMALLER = 1, 0, -1


def bf16_round(x):
    """float64 values of bf16(fl32(x)), round to nearest even (torch's conversion)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.to(torch.float64).numpy()


def table64(t):
    return t.detach().cpu().to(torch.float64).numpy()


# ---- 1.1 -------------------------------------------------------------------------------------------------------------
def max_row_norm64(ent_bf16, row_begin, m):
    """Largest Euclidean norm of rows [row_begin, row_begin + m) in float64: squares of bf16 values are exact (16
    significant bits, |v| < 2^128), their sum carries at most (d - 1) 2^-53 relative error.  A NaN or infinite entry:
    +inf (no finite bound)."""
    if m <= 0:
        return 0.0
    a = table64(ent_bf16[row_begin:row_begin + m])
    if not np.isfinite(a).all():
        return float("inf")
    return float(np.sqrt((a * a).sum(1).max()))


# ---- 1.2 -------------------------------------------------------------------------------------------------------------
def _fl32_of_sum(p1, p2):
    """Correctly rounded float32 of the EXACT p1 + p2 (float64 arrays holding exact products of bf16 values), and the
    float64 sum.  TwoSum gives the float64 sum's error; where it is not zero (the exponents lie > 37 bits apart) the
    element is rounded from the exact rational, so no double rounding is left."""
    s = p1 + p2
    bb = s - p1
    err = (p1 - (s - bb)) + (p2 - bb)
    with np.errstate(over="ignore"):
        r = s.astype(np.float32)
    for idx in zip(*np.nonzero(err != 0)):
        exact = fractions.Fraction(float(p1[idx])) + fractions.Fraction(float(p2[idx]))
        c0 = np.float32(r[idx])
        cands = [c0, np.nextafter(c0, np.float32(np.inf)), np.nextafter(c0, np.float32(-np.inf))]
        cands = [c for c in cands if np.isfinite(c)]
        dist = [abs(fractions.Fraction(float(c)) - exact) for c in cands]
        best = min(dist)
        tied = [c for c, dd in zip(cands, dist) if dd == best]
        r[idx] = tied[0] if len(tied) == 1 else [c for c in tied if (c.view(np.uint32) & 1) == 0][0]
    return r, s


def split_queries64(model, ent, rel, s, p, o):
    """{"sp": (q_hi, q_lo, q), "po": (q_hi, q_lo, q)}: float64 [n, d] arrays in the table rows' own layout (ComplEx:
    [re | im]); "sp" scores objects (the dot product with an entity row is score(s, p, that entity)), "po" subjects.

    q is the exact query up to float64 rounding, hi = bf16(fl32(q)), lo = bf16(fl32(q) - hi), the difference exact.
    DistMult: q = e r is ONE product of two bf16 values -- exact in float32, so hi and lo are the kernel's bits.
    ComplEx: q = a b +- c d with both products exact in float32; fl32(q) here is the correctly rounded exact sum.  Any
    float32 evaluation that rounds this sum once -- an fma on one exact product, or a plain add of the two exact
    products -- gives the same bits; `margin64` still carries a term for a float32 query one rounding away."""
    E, Rm = table64(ent), table64(rel)
    s, p, o = (np.asarray(x).astype(np.int64) for x in (s, p, o))
    es, eo, r = E[s], E[o], Rm[p]
    out = {}
    if model == "distmult":
        for side, a in (("sp", es), ("po", eo)):
            q = a * r
            out[side] = (q.astype(np.float32), q)
    elif model == "complex":
        h = E.shape[1] // 2
        a0, a1, r0, r1 = es[:, :h], es[:, h:], r[:, :h], r[:, h:]
        re32, re64 = _fl32_of_sum(a0 * r0, -(a1 * r1))
        im32, im64 = _fl32_of_sum(a1 * r0, a0 * r1)
        out["sp"] = (np.concatenate([re32, im32], 1), np.concatenate([re64, im64], 1))
        a0, a1 = eo[:, :h], eo[:, h:]
        re32, re64 = _fl32_of_sum(r0 * a0, r1 * a1)
        im32, im64 = _fl32_of_sum(r0 * a1, -(r1 * a0))
        out["po"] = (np.concatenate([re32, im32], 1), np.concatenate([re64, im64], 1))
    else:
        raise ValueError(model)
    res = {}
    for side, (q32, q64) in out.items():
        hi = bf16_round(q32)
        lo = bf16_round(q32.astype(np.float64) - hi)
        res[side] = (hi, lo, q64)
    return res


# ---- scores and the margin -------------------------------------------------------------------------------------------
def score_parts64(q_hi, q_lo, tab):
    """Both chains in float64 and the sums of absolute products their rounding bounds need.  The chains are kept
    apart (x64 = x_hi + x_lo) so that an infinite table entry gives what the kernel's two chains give (inf - inf = NaN)."""
    with np.errstate(all="ignore"):
        return types.SimpleNamespace(
            x_hi=q_hi @ tab.T, x_lo=q_lo @ tab.T, a_hi=np.abs(q_hi) @ np.abs(tab).T, a_lo=np.abs(q_lo) @ np.abs(tab).T,
            K=tab.shape[1])


def allowed32(t32, atol, rtol):
    """(t, allowed) as float64 arrays holding the kernel's float32 values: t NaN -> -inf, then
    fl32(fl32(atol) + |fl32(fl32(rtol) t)|) (common.hpp: is_close; the |.| between product and sum rules out an fma)."""
    t = np.asarray(t32, dtype=np.float32).copy()
    t[np.isnan(t)] = -np.inf
    with np.errstate(all="ignore"):
        al = np.float32(atol) + np.abs(np.float32(rtol) * t)
    return t.astype(np.float64), al.astype(np.float64)


def margin64(parts, t, model):
    """(e, e_hi): bounds on |x_kernel - x64| and |x_hi_kernel - x_hi64|, including the rounding of the kernel's
    subtraction of t.  Derivation (u = 2^-24, first-order terms bounded from above, nothing fitted):

    * a chain sums K exactly representable products in float32 in some order (matrix-core blocks): K - 1 additions,
      each with relative error <= u, so |chain - exact| <= gamma_{K-1} S <= K u S with S = sum_k |q_k t_jk|
      (gamma_{K-1} = (K-1)u / (1 - (K-1)u) <= K u as long as K (K-1) u <= 1, i.e. K < 4096).  One such term per chain:
          e_acc = K u (S_hi + S_lo);
    * x = fl(x_hi + x_lo): u |x_hi_k + x_lo_k| <= u (|x_hi| + |x_lo| + e_acc) = e_add;
    * the comparison rounds x - t: u |x_k - t| <= u (|x64 - t| + e_acc + e_add) = e_sub (t is the float32 the
      kernel is handed, allowed the float32 it computes: no error of their own);
    * ComplEx: a float32 query element one rounding (2^-24 |q_k|, twice for two evaluations) off the one used here
      moves the score by at most 2 u sum_k |q_k t_jk| <= 2 u (S_hi + S_lo) = e_q.  (split_queries64 explains why this
      term is slack on top of the bound, not a correction that is needed.)

    e = e_acc + e_add + e_sub + e_q; for the q_hi chain alone e_hi = K u S_hi + u (|x_hi - t| + K u S_hi) (+ e_q)."""
    K = parts.K
    assert K * (K - 1) * U <= 1.0
    T = t[:, None]
    with np.errstate(all="ignore"):
        e_acc = K * U * (parts.a_hi + parts.a_lo)
        e_add = U * (np.abs(parts.x_hi) + np.abs(parts.x_lo) + e_acc)
        e_sub = U * (np.abs(parts.x_hi + parts.x_lo - T) + e_acc + e_add)
        e_q = 2 * U * (parts.a_hi + parts.a_lo) if model == "complex" else 0.0
        e = e_acc + e_add + e_sub + e_q
        eh = K * U * parts.a_hi
        e_hi = eh + U * (np.abs(parts.x_hi - T) + eh) + e_q
    return e, e_hi


def _classify(x, e, t, allowed):
    """Class of every score against its row's tie band and what the margin leaves open.

    With d = x - t: certainly greater  d - allowed >  e;  certainly not greater  d - allowed <= -e;
                    certainly smaller  d + allowed < -e;  certainly not smaller  d + allowed >=  e
    (|x_kernel - x| <= e, so each implies the kernel's own comparison; with e = 0 they are the rule itself and a score
    exactly on an edge is close).  Where x, t, allowed or e is not finite there is no margin to apply: the rule is
    evaluated literally (x == t is close; a non-finite |x - t| is not)."""
    with np.errstate(all="ignore"):
        x = np.where(np.isnan(x), -np.inf, x)
        T, A = t[:, None], allowed[:, None]
        fin = np.isfinite(x) & np.isfinite(T) & np.isfinite(A) & np.isfinite(e)
        d = x - T
        gt_c, ngt_c = fin & (d - A > e), fin & (d - A <= -e)
        lt_c, nlt_c = fin & (d + A < -e), fin & (d + A >= e)
        err = np.abs(d)
        close_l = (x == T) | (np.isfinite(err) & (err <= A))
        gt_l = (x > T) & ~close_l
        lt_l = ~close_l & ~gt_l
    nf = ~fin
    greater, smaller = gt_c | (nf & gt_l), lt_c | (nf & lt_l)
    close = (ngt_c & nlt_c) | (nf & close_l)
    cls = np.where(greater, GREATER, np.where(smaller, SMALLER, CLOSE)).astype(np.int8)
    return types.SimpleNamespace(cls=cls, certain=greater | close | smaller, greater=greater, close=close,
                                 und_up=fin & ~gt_c & ~ngt_c, und_dn=fin & ~lt_c & ~nlt_c)


def filter_masks(filters, n, m, col_begin, true_col):
    """[K] bool [n, m]: column j of the slice is removed from ranking k + 1 of row i.  filters: [(begin [n], end [n],
    vals)] with GLOBAL column ids; ids outside the slice and the row's own target are ignored."""
    out = []
    for beg, end, vals in filters:
        mk = np.zeros((n, m), bool)
        for i in range(n):
            c = np.asarray(vals[int(beg[i]):int(end[i])], dtype=np.int64)
            c = c[(c != int(true_col[i])) & (c >= col_begin) & (c < col_begin + m)] - col_begin
            mk[i, c] = True
        out.append(mk)
    return out


def _per_ranking(val, masks):
    """[K + 1, n]: row sums of val over all columns (raw) and over the columns each filter set keeps."""
    return np.stack([val.sum(1)] + [(val & ~mk).sum(1) for mk in masks]).astype(np.int64)


# ---- 1.3 -------------------------------------------------------------------------------------------------------------
def count_bounds_from_scores(x, e, t32, atol, rtol, filters, true_col, col_begin):
    """Closed intervals of the counts from float64 scores x [n, m] of the slice whose first column is `col_begin` and a
    bound e [n, m] (or a scalar) on |x_kernel - x|.  -> rank_min, rank_max, ties_min, ties_max: int64 [K + 1, n] (row
    0 raw, row k + 1 without filter set k), `und` [n, m]: the undecided columns.

    A filtered column scores -inf: never greater, and close exactly when the true score is -inf as well."""
    n, m = x.shape
    t, al = allowed32(t32, atol, rtol)
    c = _classify(x, np.broadcast_to(np.asarray(e, dtype=np.float64), x.shape), t, al)
    masks = filter_masks(filters, n, m, col_begin, true_col)
    rank_min = _per_ranking(c.greater, masks)
    rank_max = rank_min + _per_ranking(c.und_up, masks)
    ties_min = _per_ranking(c.close, masks)
    ties_max = ties_min + _per_ranking(c.und_up | c.und_dn, masks)
    for k, mk in enumerate(masks):
        add = np.where(t == -np.inf, mk.sum(1), 0)
        ties_min[k + 1] += add
        ties_max[k + 1] += add
    return types.SimpleNamespace(rank_min=rank_min, rank_max=rank_max, ties_min=ties_min, ties_max=ties_max,
                                 und=c.und_up | c.und_dn, masks=masks)


def count_bounds64(q_hi, q_lo, tab, t32, atol, rtol, model, filters, true_col, col_begin, parts=None):
    """count_bounds_from_scores on x64 = q_hi . t_j + q_lo . t_j with the margin of `margin64`; tab = the slice's rows
    (float64), t32 = the float32 true scores the kernel is handed."""
    parts = parts or score_parts64(q_hi, q_lo, tab)
    t, _ = allowed32(t32, atol, rtol)
    e, _ = margin64(parts, t, model)
    with np.errstate(all="ignore"):
        x = parts.x_hi + parts.x_lo
    return count_bounds_from_scores(x, e, t32, atol, rtol, filters, true_col, col_begin)


# ---- 1.5 -------------------------------------------------------------------------------------------------------------
def classify_pairs(parts, q_lo, t32, atol, rtol, model, tmax64):
    """Per pair: class of x_hi alone and of x (GREATER / CLOSE / SMALLER), whether each is certain (farther than its
    margin from every edge), and `out_hi` = (|x_hi - t| - allowed) / B_i, B_i = ||q_lo_i|| tmax64: how far x_hi lies
    outside the plain tie band in units of the Cauchy-Schwarz bound (negative: inside)."""
    t, al = allowed32(t32, atol, rtol)
    e, e_hi = margin64(parts, t, model)
    with np.errstate(all="ignore"):
        x = parts.x_hi + parts.x_lo
        B = np.linalg.norm(q_lo, axis=1) * tmax64
        out_hi = (np.abs(parts.x_hi - t[:, None]) - al[:, None]) / B[:, None]
    ch, cx = _classify(parts.x_hi, e_hi, t, al), _classify(x, e, t, al)
    return types.SimpleNamespace(cls_hi=ch.cls, cert_hi=ch.certain, cls_x=cx.cls, cert_x=cx.certain, out_hi=out_hi,
                                 B=B, e=e, e_hi=e_hi, t=t, allowed=al, x=x, x_hi=parts.x_hi, und=cx.und_up | cx.und_dn)


def discriminating(cp, true_local):
    """Pairs that tell a bound too small by up to 4x: both classes certain and different, x_hi more than B_i / 4
    outside the plain band (a band launch whose bound fell below that counts them from x_hi alone: wrongly).  The
    row's own target is no such pair."""
    dm = cp.cert_hi & cp.cert_x & (cp.cls_hi != cp.cls_x) & (cp.out_hi > 0.25)
    for i, j in enumerate(true_local):
        if 0 <= j < dm.shape[1]:
            dm[i, j] = False
    return dm


def band_membership(cp, scale=1.0):
    """(certainly inside, possibly inside) the band launch's widened band when its table factor is `scale` x the true
    max norm.  The launch widens allowed_i by band = 1.001 fl(||q_lo_i|| tmax_k) + 2^-21 (|t| + allowed + band) with
    max64 <= tmax_k <= 1.002 max64 (tested on its own) and a float32 norm of q_lo within (d + 2) u of the exact one,
    so  scale B_i <= band <= 1.0035 scale B_i + 2^-20 (|t| + allowed + B_i);  its x_hi lies within e_hi of x_hi64."""
    with np.errstate(all="ignore"):
        dist = np.abs(cp.x_hi - cp.t[:, None]) - cp.allowed[:, None]
        B = cp.B[:, None]
        sure = dist <= scale * B - cp.e_hi
        maybe = dist <= 1.0035 * scale * B + 2.0 ** -20 * (np.abs(cp.t) + cp.allowed + cp.B)[:, None] + cp.e_hi
    return sure, maybe


def scaled_band_diff(cp, masks, scale, which=GREATER):
    """Interval [lo, hi] (int64 [K + 1, n] each) of (count with a band `scale` x too small) - (true count), for the
    rank (which = GREATER) or the ties (which = CLOSE): a pair certainly outside the shrunken band is counted by the
    class of x_hi, a pair inside by that of x; whatever is not certain widens the interval by one."""
    sure_in, maybe_in = band_membership(cp, scale)
    outside = ~maybe_in
    hi_g, x_g = cp.cls_hi == which, cp.cls_x == which
    settled = (sure_in & cp.cert_x) | (outside & cp.cert_hi & cp.cert_x)
    diff = np.where(outside & settled, hi_g.astype(np.int64) - x_g.astype(np.int64), 0)
    mid = _per_ranking(diff > 0, masks) - _per_ranking(diff < 0, masks)
    loose = _per_ranking(~settled, masks)
    return mid - loose, mid + loose


# ---- 1.4 -------------------------------------------------------------------------------------------------------------
def plant_aligned_rows(tab, q_hi, q_lo, t, allowed, plan, tmax_of):
    """Overwrite entity rows so that |x_lo| reaches ~0.9 of the Cauchy-Schwarz bound.  plan: [(query row i, entity row
    j, sgn, frac)].  With u = q_lo_i / ||q_lo_i|| and w the unit vector of q_hi_i's part orthogonal to u, row j becomes
    bf16(a u + b w), a = sgn 0.9 tmax (so x_lo = a ||q_lo_i|| = sgn 0.9 B_i) and b such that
        x_hi = a (q_hi . u) + b (q_hi . w) = t_i - sgn (allowed_i + frac B_i):
    x_hi alone is frac B_i outside the plain band on one side, x = x_hi + x_lo is (0.9 - frac) B_i outside it on the
    OTHER side.  sgn = +1: x_hi smaller, x greater; sgn = -1: x_hi greater, x smaller.  a^2 + b^2 <= (0.995 tmax)^2
    keeps the row -- after its bf16 rounding, at most 2^-9 relative -- below the slice's max norm tmax = tmax_of(j).
    -> the entries of `plan` that were planted (one whose b would break the norm limit is left out)."""
    done = []
    for i, j, sgn, frac in plan:
        co = aligned_coeffs(q_hi[i], q_lo[i], t[i], allowed[i], sgn, frac, tmax_of(j))
        if co is None:
            continue
        a, b, u, w = co
        tab[j] = bf16_round(a * u + b * w)
        done.append((i, j, sgn, frac))
    return done


def aligned_coeffs(q_hi, q_lo, t, allowed, sgn, frac, tm):
    """(a, b, u, w) of plant_aligned_rows for one query row and one planted column, or None where q_lo = 0, q_hi is
    parallel to it, or b breaks the norm limit."""
    nl = np.linalg.norm(q_lo)
    if not nl > 0:
        return None
    u = q_lo / nl
    h = q_hi - (q_hi @ u) * u
    nh = np.linalg.norm(h)
    if not nh > 0:
        return None
    a = sgn * 0.9 * tm
    b = (t - sgn * (allowed + frac * nl * tm) - a * (q_hi @ u)) / nh
    if a * a + b * b > (0.995 * tm) ** 2:
        return None
    return a, b, u, h / nh


# ---- the test inputs (shared by the CPU conditions and the GPU tests: same seeds, same code) --------------------------
ATOL, RTOL = 1e-5, 1e-4    # the reference implementation's tie tolerances (what the evaluator passes)
SPLIT_AT = 2049            # two entity chunks: ((0, 2049), (2049, E)) -- the first one ends inside a 64-column tile

PLANTED_CASES = [
    # model, E, R, d, n, K, two entity chunks.  Every level the band path distinguishes appears: d 256 / 512, both
    # scorers, no / two filter sets, n = 1 / 33 / 100 / 300 (ragged 32-row groups, both halves of a 64-row fragment
    # group, two 256-row chunks), E ~ 2,100 / 4,099, one / two entity chunks with max norms 2x apart.
    ("distmult", 2100, 5, 256, 1, 0, False),
    ("complex", 2100, 5, 256, 33, 2, False),
    ("distmult", 2111, 7, 256, 100, 2, False),
    ("complex", 4099, 7, 256, 300, 2, True),
    ("distmult", 4099, 7, 256, 300, 0, True),
    ("complex", 2100, 5, 512, 1, 2, False),
    ("distmult", 2100, 5, 512, 33, 0, False),
    ("complex", 4099, 7, 512, 100, 0, True),
    ("distmult", 4099, 7, 512, 300, 2, True),
    ("complex", 2100, 5, 512, 300, 2, False),
    ("distmult", 4099, 7, 256, 33, 2, True),
    ("complex", 4099, 7, 256, 100, 0, False),
]
PLANT_ROWS = (0, 7, 31, 32, 45, 63, 64, 98, 130, 191, 256, 290)   # (and always the last row)

_CASES = {}
SEED0 = 2000   # (with this base every case meets the conditions test_rank_band_ref_cpu.py checks: the reference's own verdict)


def build_case(idx):
    """Tables, triples, filters and planted rows of PLANTED_CASES[idx]; cached, treated as read-only."""
    if idx in _CASES:
        return _CASES[idx]
    model, E, R, d, n, K, two = PLANTED_CASES[idx]
    seed = SEED0 + idx
    g = torch.Generator().manual_seed(seed)
    ent = (torch.randn(E, d, generator=g) * 0.3).to(torch.bfloat16)
    rel = (torch.randn(R, d, generator=g) * 0.3).to(torch.bfloat16)
    rng = np.random.default_rng(seed)
    chunks = ((0, SPLIT_AT), (SPLIT_AT, E)) if two else ((0, E),)
    tab = table64(ent)
    s = rng.choice(E, n, replace=False).astype(np.int64)   # distinct (s, p) keys
    p = rng.integers(0, R, n).astype(np.int64)
    # one designated row per chunk with exactly the largest norm: 1.05 x the chunk's natural maximum, in the first of
    # two chunks 2.3 x (the chunks' bounds then differ by more than 2x)
    free = np.setdiff1d(np.arange(E), s)
    designated = []
    for c, (lo, hi) in enumerate(chunks):
        j = int(free[(free >= lo) & (free < hi)][11])
        nat = np.sqrt((tab[lo:hi] ** 2).sum(1).max())
        f = 2.3 if (two and c == 0) else 1.05
        tab[j] = bf16_round(tab[j] * (f * nat / np.linalg.norm(tab[j])))
        designated.append(j)
    # true objects: the best ordinary entity of (s, p) -- a trained model's triples; the same score sits in the tail
    # of (p, o)'s row, so few random columns come near the tie band's edges
    ent1 = torch.from_numpy(tab).to(torch.bfloat16)
    q = split_queries64(model, ent1, rel, s, p, s)["sp"]
    sc = (q[0] + q[1]) @ tab.T
    sc[:, designated] = -np.inf    # (a designated row as an object would give a (p, o) query of more than twice the norm)
    o = np.argmax(sc, axis=1).astype(np.int64)
    Q = split_queries64(model, ent1, rel, s, p, o)
    true_col = {"sp": o, "po": s}
    t_ref = {}
    for side in ("sp", "po"):
        hi_, lo_, _ = Q[side]
        rows = tab[true_col[side]]
        t_ref[side] = ((hi_ * rows).sum(1) + (lo_ * rows).sum(1)).astype(np.float32)
    # the plan: rows of both halves of a 64-row group, of both 256-row chunks, the last row; per row ONE kind
    tmax_nat = [float(np.sqrt((tab[lo:hi] ** 2).sum(1).max())) for lo, hi in chunks]
    chunk_of = lambda j: 0 if (not two or j < SPLIT_AT) else 1
    prow = sorted({r for r in PLANT_ROWS if r < n} | {n - 1})
    per_row = 4 if n >= 33 else 12    # (one row: 4 columns could not give 8 pairs)
    fracs = np.linspace(0.34, 0.72, per_row)
    used = set(s.tolist()) | set(o.tolist()) | set(designated)
    pool = [j for j in rng.permutation(E).tolist() if j not in used]
    pools = [[j for j in pool if chunk_of(j) == c] for c in range(len(chunks))]
    planted = {"sp": [], "po": []}
    for side_i, side in enumerate(("sp", "po")):
        hi_, lo_, _ = Q[side]
        t64, al = allowed32(t_ref[side], ATOL, RTOL)
        # kinds alternate over the planted rows; a row on which the kind in turn would break the norm limit (q_hi has a
        # component along q_lo, which a has to make up for) takes the other kind
        sgn_of = []
        for ri, i in enumerate(prow):
            want = 1 if (ri + side_i) % 2 == 0 else -1
            ok = [sg for sg in (want, -want) if all(aligned_coeffs(hi_[i], lo_[i], t64[i], al[i], sg, f, tm) is not None
                                                   for f in (fracs[0], fracs[-1]) for tm in tmax_nat)]
            sgn_of.append(ok[0] if ok else want)
        plan = []
        for ri, i in enumerate(prow):
            for c in range(per_row):
                ch = (c + ri) % len(chunks)
                plan.append((i, pools[ch].pop(), sgn_of[ri], float(fracs[c])))
        planted[side] = plant_aligned_rows(tab, hi_, lo_, t64, al, plan, lambda j: tmax_nat[chunk_of(j)])
    ent2 = torch.from_numpy(tab).to(torch.bfloat16)
    assert np.array_equal(table64(ent2), tab)
    tmax64 = [max_row_norm64(ent2, lo, hi - lo) for lo, hi in chunks]
    assert tmax64 == tmax_nat, "a planted row raised a chunk's max norm"
    for c, (lo, hi) in enumerate(chunks):
        assert int(np.argmax((tab[lo:hi] ** 2).sum(1))) + lo == designated[c]
    # K nested filter sets: a few random columns, the row's target in most, an empty range now and then; of a row's
    # planted columns the first is in both sets, the second in the second set only, the others in none
    filters = {}
    for side in ("sp", "po"):
        by_row = {}
        for i, j, _, _ in planted[side]:
            by_row.setdefault(i, []).append(j)
        sets, prev = [], [np.zeros(0, np.int64)] * n
        for k in range(K):
            begin, end, vals = np.zeros(n, np.int64), np.zeros(n, np.int64), []
            for i in range(n):
                v = rng.choice(E, size=int(rng.integers(0, 6)), replace=False)
                if rng.random() < 0.8:
                    v = np.append(v, true_col[side][i])
                mine = by_row.get(i, [])
                v = np.setdiff1d(np.concatenate([v, prev[i]]), np.asarray(mine, np.int64))
                v = np.union1d(v, np.asarray(mine[:k + 1], np.int64)).astype(np.int64)
                if i % 7 == 3 and k == 0 and not mine:
                    v = np.zeros(0, np.int64)
                prev[i] = v
                begin[i] = len(vals)
                vals.extend(v.tolist())
                end[i] = len(vals)
            sets.append((begin, end, np.asarray(vals if vals else [0], np.int64)))
        filters[side] = sets
    case = types.SimpleNamespace(idx=idx, model=model, E=E, R=R, d=d, n=n, K=K, chunks=chunks, ent=ent2, rel=rel, s=s,
                                 p=p, o=o, true_col=true_col, t_ref=t_ref, Q=Q, tab=tab, tmax64=tmax64,
                                 designated=designated, planted=planted, filters=filters, _parts={})
    _CASES[idx] = case
    return case


def case_parts(case, side, c):
    key = (side, c)
    if key not in case._parts:
        lo, hi = case.chunks[c]
        case._parts[key] = score_parts64(case.Q[side][0], case.Q[side][1], case.tab[lo:hi])
    return case._parts[key]


def case_report(case, t=None, atol=ATOL, rtol=RTOL):
    """Everything the tests ask of a case, per side and entity chunk, for true scores `t` = {"sp": float32 [n], "po":
    ...} (default: the reference's own, case.t_ref): count intervals, the classes, discriminating pairs, pairs
    certainly / possibly inside the widened band."""
    t = t or case.t_ref
    rep = {}
    for side in ("sp", "po"):
        for c, (lo, hi) in enumerate(case.chunks):
            parts = case_parts(case, side, c)
            cp = classify_pairs(parts, case.Q[side][1], t[side], atol, rtol, case.model, case.tmax64[c])
            b = count_bounds_from_scores(cp.x, cp.e, t[side], atol, rtol, case.filters[side], case.true_col[side], lo)
            disc = discriminating(cp, case.true_col[side] - lo)
            sure, maybe = band_membership(cp)
            rep[side, c] = types.SimpleNamespace(cp=cp, bounds=b, disc=disc, listed_sure=sure, listed_maybe=maybe)
    return rep


def report_totals(case, rep):
    """(discriminating, certainly listed, possibly listed, undecided) pairs per side over the chunks -- for messages."""
    out = {}
    for side in ("sp", "po"):
        rs = [rep[side, c] for c in range(len(case.chunks))]
        out[side] = dict(discriminating=int(sum(r.disc.sum() for r in rs)), listed_sure=int(sum(r.listed_sure.sum() for r in rs)),
                         listed_maybe=int(sum(r.listed_maybe.sum() for r in rs)), undecided=int(sum(r.bounds.und.sum() for r in rs)))
    return out


def total_bounds(case, rep):
    """Intervals of the counts accumulated over the entity chunks, as the kernels accumulate them: int64
    [side (sp, po), rank | ties, K + 1, n] for the minimum and the maximum."""
    mn = np.zeros((2, 2, case.K + 1, case.n), np.int64)
    mx = np.zeros_like(mn)
    for si, side in enumerate(("sp", "po")):
        for c in range(len(case.chunks)):
            b = rep[side, c].bounds
            mn[si, 0] += b.rank_min
            mn[si, 1] += b.ties_min
            mx[si, 0] += b.rank_max
            mx[si, 1] += b.ties_max
    return mn, mx
