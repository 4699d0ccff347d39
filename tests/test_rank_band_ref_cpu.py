"""The float64 reference of the parity-mode ranking counts (_rank_band_ref.py) and the inputs it builds for
test_gpu_rank_band_bound.py, checked without a GPU: count_bounds64 against a brute-force loop, and -- for EVERY GPU
case, same seeds, same code -- the conditions that make those inputs worth running: pairs whose x_lo comes near the
Cauchy-Schwarz bound exist where the band launch could go wrong (both halves of a 64-row fragment group, the last row of
a ragged batch), no list fills, and the margin leaves next to nothing undecided."""
import numpy as np
import pytest
import torch

import _rank_band_ref as R


# ---- 2.3: count_bounds64 against a brute-force loop -------------------------------------------------------------------
def _brute(x, e, t32, atol, rtol, filters, true_col, col_begin):
    """The rule of kge_rank_counts, one pair at a time, with every comparison widened by e."""
    n, m = x.shape
    K = len(filters)
    out = np.zeros((4, K + 1, n), np.int64)   # rank_min, rank_max, ties_min, ties_max
    for i in range(n):
        t = np.float32(t32[i])
        if np.isnan(t):
            t = np.float32(-np.inf)
        with np.errstate(all="ignore"):
            allowed = float(np.float32(atol) + np.abs(np.float32(rtol) * t))
        t = float(t)
        for k in range(K + 1):
            removed = set()
            if k > 0:
                b, en, v = filters[k - 1]
                removed = {int(c) - col_begin for c in v[b[i]:en[i]] if int(c) != int(true_col[i])}
            for j in range(m):
                xv = float(x[i, j])
                if j in removed:
                    xv = -np.inf
                if np.isnan(xv):
                    xv = -np.inf
                ee = float(e[i, j])
                if not (np.isfinite(xv) and np.isfinite(t) and np.isfinite(allowed) and np.isfinite(ee)):
                    with np.errstate(all="ignore"):
                        err = abs(xv - t)
                    close = xv == t or (np.isfinite(err) and err <= allowed)
                    g = xv > t and not close
                    out[0, k, i] += g
                    out[1, k, i] += g
                    out[2, k, i] += close
                    out[3, k, i] += close
                    continue
                dd = xv - t
                g_sure, g_not = dd - allowed > ee, dd - allowed <= -ee
                l_sure, l_not = dd + allowed < -ee, dd + allowed >= ee
                out[0, k, i] += g_sure
                out[1, k, i] += not g_not
                out[2, k, i] += g_not and l_not
                out[3, k, i] += not (g_sure or l_sure)
    return out


def _tiny(seed, n=5, m=23, K=2, col_begin=7):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, m))
    t32 = rng.normal(size=n).astype(np.float32)
    true_col = rng.integers(col_begin, col_begin + m, n)
    filters = []
    for k in range(K):
        beg, end, vals = np.zeros(n, np.int64), np.zeros(n, np.int64), []
        for i in range(n):
            v = rng.choice(col_begin + m + 9, size=int(rng.integers(0, 8)), replace=False)   # some outside the chunk
            if i % 2 == 0:
                v = np.union1d(v, [true_col[i]])                                              # the filtered true column
            beg[i] = len(vals)
            vals.extend(int(c) for c in v)
            end[i] = len(vals)
        filters.append((beg, end, np.asarray(vals if vals else [0], np.int64)))
    return x, t32, true_col, filters, col_begin


def _same(b, want, what):
    got = np.stack([b.rank_min, b.rank_max, b.ties_min, b.ties_max])
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


def test_count_bounds_equal_a_brute_force_loop():
    for seed in range(4):
        x, t32, true_col, filters, cb = _tiny(seed)
        atol, rtol = 0.05, 0.01
        for e in (0.0, 0.03):
            ee = np.full(x.shape, e)
            b = R.count_bounds_from_scores(x, ee, t32, atol, rtol, filters, true_col, cb)
            _same(b, _brute(x, ee, t32, atol, rtol, filters, true_col, cb), (seed, e))
            assert (b.rank_min <= b.rank_max).all() and (b.ties_min <= b.ties_max).all()
            if e == 0.0:
                assert np.array_equal(b.rank_min, b.rank_max) and np.array_equal(b.ties_min, b.ties_max)
            else:
                assert int(b.und.sum()) > 0


def test_count_bounds_on_ties_exactly_on_an_edge():
    """allowed = 0.25 + |0.5 * 2| = 1.25 exactly (float32 and float64 agree): scores exactly on an edge are close, 2^-40
    beyond is not; with a margin both are undecided for that edge only."""
    t32 = np.asarray([2.0], np.float32)
    up, dn = 3.25 + 2.0 ** -40, 0.75 - 2.0 ** -40   # (exact in float64, and so are their differences from t)
    x = np.asarray([[3.25, up, 0.75, dn, 2.0, 10.0, -10.0]])
    b = R.count_bounds_from_scores(x, 0.0, t32, 0.25, 0.5, [], np.asarray([4]), 0)
    assert (int(b.rank_min[0, 0]), int(b.rank_max[0, 0]), int(b.ties_min[0, 0]), int(b.ties_max[0, 0])) == (2, 2, 3, 3)
    b = R.count_bounds_from_scores(x, 1e-9, t32, 0.25, 0.5, [], np.asarray([4]), 0)
    assert (int(b.rank_min[0, 0]), int(b.rank_max[0, 0]), int(b.ties_min[0, 0]), int(b.ties_max[0, 0])) == (1, 3, 1, 5)
    _same(b, _brute(x, np.full(x.shape, 1e-9), t32, 0.25, 0.5, [], np.asarray([4]), 0), "edge")


def test_count_bounds_with_nan_and_infinite_scores():
    inf, nan = np.inf, np.nan
    x = np.asarray([[inf, -inf, nan, 0.5, 1.0, 3.0]] * 5)
    t32 = np.asarray([1.0, inf, -inf, nan, 0.9999], np.float32)
    true_col = np.asarray([4, 0, 1, 2, 4])
    filters = [(np.arange(5), np.arange(5) + 1, np.asarray([5, 0, 5, 2, 3]))]   # rows 1, 3 filter their own target
    for rtol in (0.0, 1e-3):   # rtol = 0 with an infinite true score: allowed = 0 * inf = NaN, nothing is close but x == t
        for e in (0.0, 1e-3):
            ee = np.full(x.shape, e)
            b = R.count_bounds_from_scores(x, ee, t32, 1e-5, rtol, filters, true_col, 0)
            _same(b, _brute(x, ee, t32, 1e-5, rtol, filters, true_col, 0), (rtol, e))
    b = R.count_bounds_from_scores(x, 0.0, t32, 1e-5, 1e-3, filters, true_col, 0)
    # t = 1: +inf and 3 greater, 1.0 close.  t = +inf: only +inf close.  t = -inf and t = NaN (= -inf): -inf and NaN
    # close, the four others greater -- and the filtered column joins the ties (-inf is close to -inf)
    assert b.rank_min[0].tolist() == [2, 0, 4, 4, 2] and b.ties_min[0].tolist() == [1, 1, 2, 2, 1]
    assert b.rank_min[1].tolist() == [1, 0, 3, 4, 2] and b.ties_min[1].tolist() == [1, 1, 3, 2, 1]


def test_count_bounds64_from_tables_with_an_infinite_entry():
    """Both chains apart: q_hi = 1, q_lo = -2^-9 against an infinite entry is +inf - inf = NaN = -inf for the kernel,
    not (q_hi + q_lo) * inf = +inf."""
    q_hi, q_lo = np.asarray([[1.0, 1.0]]), np.asarray([[-2.0 ** -9, 0.0]])
    tab = np.asarray([[np.inf, 0.0], [1.0, 1.0], [0.0, np.inf]])
    b = R.count_bounds64(q_hi, q_lo, tab, np.asarray([1.0], np.float32), 1e-5, 1e-4, "distmult", [], np.asarray([1]), 0)
    assert int(b.rank_min[0, 0]) == int(b.rank_max[0, 0]) == 1   # only the column with +inf in both chains' finite part


# ---- 1.1 / 1.2 --------------------------------------------------------------------------------------------------------
def test_max_row_norm64():
    ent = torch.zeros(6, 8).bfloat16()
    ent[1, :] = 2.0
    ent[4, 0] = 100.0
    assert R.max_row_norm64(ent, 0, 6) == 100.0 and R.max_row_norm64(ent, 0, 4) == float(np.sqrt(32.0))
    assert R.max_row_norm64(ent, 2, 2) == 0.0 and R.max_row_norm64(ent, 5, 0) == 0.0
    ent[3, 3] = float("nan")
    assert R.max_row_norm64(ent, 0, 6) == float("inf") and R.max_row_norm64(ent, 4, 2) == 100.0
    big = torch.full((1, 8), 1e30).bfloat16()   # squares beyond float32: still finite here
    assert np.isfinite(R.max_row_norm64(big, 0, 1)) and R.max_row_norm64(big, 0, 1) > 2.8e30


@pytest.mark.parametrize("model", ["distmult", "complex"])
def test_split_queries64(model):
    g = torch.Generator().manual_seed(3)
    ent, rel = (torch.randn(50, 64, generator=g) * 0.3).bfloat16(), (torch.randn(4, 64, generator=g) * 0.3).bfloat16()
    ent[0, 0], ent[0, 32] = 2.0 ** -30, 1.5   # ComplEx: two products 2^-60 and O(1) -- the float64 sum is inexact
    rel[0, 0], rel[0, 32] = 2.0 ** -30, 1.0
    s, p, o = np.arange(10), np.arange(10) % 4, np.arange(10, 20)
    Q = R.split_queries64(model, ent, rel, s, p, o)
    E, Rm = R.table64(ent), R.table64(rel)
    for side, own, other in (("sp", s, o), ("po", o, s)):
        hi, lo, q = Q[side]
        # the layout is the table rows' own: the query against the other entity's row is the triple's score
        if model == "distmult":
            want = (E[s] * Rm[p] * E[o]).sum(1)
        else:
            h = 32
            sr, si, pr, pi, orr, oi = E[s][:, :h], E[s][:, h:], Rm[p][:, :h], Rm[p][:, h:], E[o][:, :h], E[o][:, h:]
            want = (sr * pr * orr + si * pr * oi + sr * pi * oi - si * pi * orr).sum(1)
        assert np.allclose((q * E[other]).sum(1), want, rtol=1e-12, atol=1e-14), side
        q32 = q.astype(np.float32).astype(np.float64)
        # hi and lo are bf16 values, hi the rounding of q, hi + lo within half a bf16 ulp of lo of fl32(q)
        assert np.array_equal(R.bf16_round(hi), hi) and np.array_equal(R.bf16_round(lo), lo)
        assert (np.abs(q - hi) <= 2.0 ** -8 * np.abs(q)).all()
        assert (np.abs(q32 - hi - lo) <= 2.0 ** -17 * np.abs(q) + 1e-300).all()
        if model == "distmult":
            assert np.array_equal(q32, q)   # one product of two bf16 values: exact


# ---- 2.2: the GPU cases' inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(R.PLANTED_CASES)))
def test_planted_inputs_meet_their_conditions(idx):
    case = R.build_case(idx)
    rep = R.case_report(case)
    tot = R.report_totals(case, rep)
    msg = (R.PLANTED_CASES[idx], tot)
    n, nch = case.n, len(case.chunks)
    # the construction: planted rows reach ~0.9 of the bound and sit in every chunk; one row has exactly the largest norm
    for c, (lo, hi) in enumerate(case.chunks):
        norms = np.sqrt((case.tab[lo:hi] ** 2).sum(1))
        assert int(np.argmax(norms)) + lo == case.designated[c] and (np.sort(norms)[-2] < norms.max()), msg
    if nch == 2:
        assert case.tmax64[0] >= 2.0 * case.tmax64[1], (msg, case.tmax64)
    for side in ("sp", "po"):
        ratios = []
        for i, j, sgn, _ in case.planted[side]:
            c = 0 if (nch == 1 or j < R.SPLIT_AT) else 1
            ratios.append(sgn * case_x_lo(case, side, c)[i, j - case.chunks[c][0]] / rep[side, c].cp.B[i])
            assert any(lo <= j < hi for lo, hi in case.chunks)
        assert len(ratios) >= 8 and min(ratios) > 0.85 and max(ratios) < 0.95, (msg, side, min(ratios), max(ratios))
        if nch == 2:
            assert {0 if j < R.SPLIT_AT else 1 for _, j, _, _ in case.planted[side]} == {0, 1}, msg
        if case.K:   # some planted columns are filtered, some are not
            filt = set(case.filters[side][case.K - 1][2].tolist())
            inside = [j in filt for _, j, _, _ in case.planted[side]]
            assert any(inside) and not all(inside), msg
        # (a) at least 8 discriminating pairs per direction
        disc_rows = np.zeros(n, bool)
        for c in range(nch):
            disc_rows |= rep[side, c].disc.any(1)
        assert tot[side]["discriminating"] >= 8, msg
        # (b) ... on rows in each half of a 64-row fragment group, (c) ... on the last real row of the batch
        rows = np.nonzero(disc_rows)[0]
        assert (rows % 64 < 32).any(), msg
        if n > 32:
            assert (rows % 64 >= 32).any(), msg
        if n > 256:
            assert (rows >= 256).any() and (rows < 256).any(), msg   # both 256-row chunks
        assert disc_rows[n - 1], msg
        # (d) per 32-row group, side and launch at most half of V8_BAND_CAP = 255 pairs possibly inside the widened band
        for c in range(nch):
            per_group = [int(rep[side, c].listed_maybe[g:g + 32].sum()) for g in range(0, n, 32)]
            assert max(per_group) <= 128, (msg, side, c, per_group)
            assert int(rep[side, c].listed_sure.sum()) <= int(rep[side, c].listed_maybe.sum())
        # (e) undecided columns: at most 2 per row, at most 1 % of all pairs
        und = sum(rep[side, c].bounds.und.sum(1) for c in range(nch))
        assert int(und.max()) <= 2 and int(und.sum()) <= 0.01 * n * case.E, (msg, side, int(und.max()))
        # every row's own target is inside its band, and certainly listed
        for i in range(n):
            j = int(case.true_col[side][i])
            c = 0 if (nch == 1 or j < R.SPLIT_AT) else 1
            assert rep[side, c].listed_sure[i, j - case.chunks[c][0]], (msg, side, i)
    # a band 4x too small is visible: on every row with a discriminating pair the predicted rank difference excludes 0
    for side in ("sp", "po"):
        lo_t = np.zeros((case.K + 1, n), np.int64)
        hi_t = np.zeros_like(lo_t)
        disc_rows = np.zeros(n, bool)
        for c in range(nch):
            r = rep[side, c]
            lo, hi = R.scaled_band_diff(r.cp, r.bounds.masks, 0.25)
            lo_t += lo
            hi_t += hi
            disc_rows |= r.disc.any(1)
        visible = (lo_t[0] > 0) | (hi_t[0] < 0)
        assert int((visible & disc_rows).sum()) >= min(4, int(disc_rows.sum())), (msg, side, lo_t[0], hi_t[0])


def case_x_lo(case, side, c):
    return R.case_parts(case, side, c).x_lo


def test_plant_aligned_rows_places_x_hi_and_x_on_opposite_sides():
    """One row by hand: x_hi = t - sgn (allowed + frac B) and x_lo = sgn 0.9 B up to the planted row's bf16 rounding
    (2^-9 per element: a few percent of B), its norm below tmax."""
    rng = np.random.default_rng(0)
    d, tm = 256, 5.0
    q = rng.normal(size=(1, d)) * 0.09
    hi = R.bf16_round(q)
    lo = R.bf16_round(q.astype(np.float32).astype(np.float64) - hi)
    tab = np.zeros((4, d))
    t, al = np.asarray([1.0]), np.asarray([1e-4])
    done = R.plant_aligned_rows(tab, hi, lo, t, al, [(0, 1, 1, 0.5), (0, 2, -1, 0.4), (0, 3, 1, 4000.0)], lambda j: tm)
    assert [x[1] for x in done] == [1, 2] and not tab[3].any()   # frac = 4000: beyond the norm limit, left out
    B = np.linalg.norm(lo[0]) * tm
    for j, sgn, frac in ((1, 1, 0.5), (2, -1, 0.4)):
        x_hi, x_lo = hi[0] @ tab[j], lo[0] @ tab[j]
        assert abs(x_lo - sgn * 0.9 * B) < 0.02 * B and abs(x_hi - (1.0 - sgn * (1e-4 + frac * B))) < 0.1 * B
        assert np.linalg.norm(tab[j]) < tm and np.array_equal(R.bf16_round(tab[j]), tab[j])
        assert sgn * (x_hi + x_lo - 1.0) > 0.25 * B and sgn * (x_hi - 1.0) < -0.25 * B
