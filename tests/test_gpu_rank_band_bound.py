"""Band-and-rescore ranking (kge_score_rank_sp_po_band, kge_eval_batch_band, kge_table_max_row_norm)
where its one inequality is tight, and the parity-mode counts against a float64 reference.

The band launch counts a pair from x_hi = q_hi . t_j alone when x_hi lies outside the tie band widened by
||q_lo_i|| max_j ||t_j|| >= |x_lo|.  On random tables |x_lo| stays 16 to 22 times below that bound, so a bound that is
too small by an order of magnitude goes unnoticed.  The inputs here (_rank_band_ref.build_case) hold entity rows aligned
with single rows' q_lo: |x_lo| ~ 0.9 of the bound, x_hi and x on opposite sides of the tie band.  Their fitness is the
reference's verdict alone (test_rank_band_ref_cpu.py, same seeds); the tests below state

  3.1  kge_table_max_row_norm >= the float64 max norm of exactly its slice, and <= 1.002 x it;
  3.2  band counts == split-kernel counts on the planted inputs, nothing dropped, lists empty;
  3.3  split and band counts inside the float64 intervals of count_bounds64 (planted and plain random inputs);
  3.4  the same inputs with the bound divided by four DO miscount, where the reference says so;
  3.5  the four-launch entry on a planted batch."""
import numpy as np
import pytest
import torch

import _rank_band_ref as R
from test_gpu_score_rank import CASES, _filters, _fused, _tables, _true_scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDES = ("sp", "po")


# ---- 3.1 -------------------------------------------------------------------------------------------------------------
M_WRAP = 4 * 2048 + 7   # the launch has at most 2,048 blocks of 4 rows: rows from 8,192 on are a block's second trip


@pytest.mark.parametrize("model,d", [("distmult", 256), ("complex", 256), ("distmult", 512), ("complex", 512)])
def test_table_max_row_norm_against_float64(model, d):
    """out >= max64 is what the band needs (never below); out <= 1.002 max64 follows from the kernel's contract:
    out = fl(1.001f * sqrtf(s2)), s2 a float32 sum of d exact squares (bf16 x bf16 has 16 significant bits).  Any
    summation order keeps s2 within (d - 1) 2^-24 <= 3.1e-5 of the exact sum, the square root halves that, sqrtf and the
    product add <= 3 2^-24, 1.001f is within 2^-24 of 1.001: out / max64 in 1.001 (1 +- 1.6e-5), inside [1, 1.002]."""
    from kge_amd import engine as eng
    N = M_WRAP + 4
    g = torch.Generator().manual_seed(d + len(model))
    base = (torch.randn(N, d, generator=g) * 0.3).to(torch.bfloat16)
    rel = (torch.randn(3, d, generator=g) * 0.3).to(torch.bfloat16).to(DEV)
    ratios = []

    def run(ent, row_begin, m, name, finite=True):
        T = eng.Tables(model, ent.to(DEV), rel, 1.0, flags=eng.FLAG_SPLIT_QUERY)
        out = float(eng.RankBand(T, 1, row_begin, row_begin + m).tmax.item())
        ref = R.max_row_norm64(ent, row_begin, m)
        if finite:
            assert np.isfinite(ref)
            assert ref <= out <= 1.002 * ref, (model, d, name, out, ref, out / ref if ref else None)
            if ref > 0:
                ratios.append((name, out / ref))
        return out

    for m in (1, 3, 4, 5, 4099, M_WRAP):
        run(base, 0, m, f"m={m}")
    for name, at in (("first", 0), ("last", M_WRAP - 1), ("wrap", 4 * 2048 + 6)):
        ent = base.clone()
        ent[2 + at] = (ent[2 + at].float() * 3.0).to(torch.bfloat16)
        # row_begin = 2 with far larger rows right before and right behind the slice: they must not count
        ent[1] = (ent[1].float() * 100.0).to(torch.bfloat16)
        ent[2 + M_WRAP] = (ent[2 + M_WRAP].float() * 100.0).to(torch.bfloat16)
        out = run(ent, 2, M_WRAP, f"largest {name}, row_begin=2")
        own = float(np.linalg.norm(R.table64(ent[2 + at])))
        assert own <= out <= 1.002 * own, (name, out, own)
        if name == "wrap":   # the slice without its last row: the next largest, not this one
            assert run(ent, 2, M_WRAP - 1, "without the last row") < own
    ent = base.clone()
    ent[4], ent[8] = (ent[4].float() * 50.0).to(torch.bfloat16), (ent[8].float() * 50.0).to(torch.bfloat16)
    run(ent, 5, 3, "m=3 between two large rows")
    assert run(torch.zeros_like(base), 0, M_WRAP, "zero table") == 0.0
    for name, val, at in (("nan", float("nan"), (4 * 2048 + 6, d - 1)), ("+inf", float("inf"), (3, 0)),
                          ("-inf", float("-inf"), (4097, 5))):
        ent = base.clone()
        ent[at] = val
        assert run(ent, 0, M_WRAP, name, finite=False) == float("inf"), name
        if at[0] > 10:
            run(ent, 0, 3, name + " outside the slice")   # finite again
    ent = base.clone()
    ent[77] = 1e20   # squares beyond float32: +inf, never a finite value below the true norm
    assert np.isfinite(R.max_row_norm64(ent, 0, 100))
    assert run(ent, 0, 100, "overflow", finite=False) == float("inf")
    print("TMAX_RATIOS", model, d, " ".join(f"{n}:{r:.7f}" for n, r in ratios))


# ---- the planted cases, run once -------------------------------------------------------------------------------------
_RUNS = {}


def _dev_inputs(eng, case):
    T = eng.Tables(case.model, case.ent.to(DEV), case.rel.to(DEV), 1.0, flags=eng.FLAG_SPLIT_QUERY)
    s, p, o = (torch.from_numpy(x).to(DEV) for x in (case.s, case.p, case.o))
    f = {side: [tuple(torch.from_numpy(x).to(DEV) for x in fs) for fs in case.filters[side]] for side in SIDES}
    return T, s, p, o, f


def _band_counts(eng, T, s, p, o, t_sp, t_po, f, chunks, K, scale=None):
    """Counts with band-and-rescore, one RankBand per chunk (its bound multiplied by `scale` first), and per chunk
    (pairs listed, pairs dropped)."""
    n = s.numel()
    got = torch.zeros(2, 2, K + 1, n, dtype=torch.int64, device=DEV)
    stats = []
    for lo, hi in chunks:
        band = eng.RankBand(T, n, lo, hi)
        if scale is not None:
            band.tmax.mul_(scale)   # a caller-owned input of the C API
        assert eng.score_rank_sp_po(T, s, p, o, t_sp, t_po, f["sp"], f["po"], R.ATOL, R.RTOL, got[0, 0], got[0, 1],
                                    got[1, 0], got[1, 1], lo, hi, band=band)
        stats.append(band.status())
        assert int(band.list.view(torch.int32).view(-1, 1024)[:, 0].abs().sum()) == 0   # every list empty again
    return got, stats


def _run(idx):
    if idx not in _RUNS:
        from kge_amd import engine as eng
        case = R.build_case(idx)
        T, s, p, o, f = _dev_inputs(eng, case)
        t_sp, t_po = _true_scores(eng, T, s, p, o)
        want = _fused(eng, T, s, p, o, t_sp, t_po, f["sp"], f["po"], case.chunks, R.ATOL, R.RTOL)
        got, stats = _band_counts(eng, T, s, p, o, t_sp, t_po, f, case.chunks, case.K)
        t = {"sp": t_sp.cpu().numpy(), "po": t_po.cpu().numpy()}
        rep = R.case_report(case, t)
        _RUNS[idx] = (case, want.cpu().numpy(), got.cpu().numpy(), stats, rep, t)
    return _RUNS[idx]


ALL = range(len(R.PLANTED_CASES))


@pytest.mark.parametrize("idx", ALL)
def test_band_counts_equal_split_counts_where_x_lo_reaches_the_bound(idx):
    case, want, got, stats, rep, t = _run(idx)
    msg = (R.PLANTED_CASES[idx], R.report_totals(case, rep), stats)
    # the inputs are what the CPU tests vouch for, also with the true scores the device computed
    for side in SIDES:
        assert sum(int(rep[side, c].disc.sum()) for c in range(len(case.chunks))) >= 8, msg
    assert np.array_equal(got, want), (msg, np.argwhere(got != want)[:5].tolist(), got[got != want][:5].tolist(),
                                       want[got != want][:5].tolist())
    for c, (listed, dropped) in enumerate(stats):
        sure = sum(int(rep[side, c].listed_sure.sum()) for side in SIDES)
        assert dropped == 0 and listed >= sure, (msg, c, listed, sure)


@pytest.mark.parametrize("idx", ALL)
def test_planted_counts_lie_inside_the_float64_intervals(idx):
    case, want, got, stats, rep, t = _run(idx)
    msg = (R.PLANTED_CASES[idx], R.report_totals(case, rep))
    # the true scores themselves: the device's t is a kernel score of the true column, within its margin of x64
    for side in SIDES:
        for i in range(case.n):
            j = int(case.true_col[side][i])
            c = 0 if (len(case.chunks) == 1 or j < R.SPLIT_AT) else 1
            cp = rep[side, c].cp
            jj = j - case.chunks[c][0]
            assert abs(float(t[side][i]) - cp.x[i, jj]) <= cp.e[i, jj], (msg, side, i)
    mn, mx = R.total_bounds(case, rep)
    for name, cnt in (("split", want), ("band", got)):
        bad = (cnt < mn) | (cnt > mx)
        assert not bad.any(), (msg, name, np.argwhere(bad)[:5].tolist(), cnt[bad][:5].tolist(), mn[bad][:5].tolist(),
                               mx[bad][:5].tolist())
    assert (want[:, 1, 0] >= 1).all()   # every row is at least close to itself (raw ranking)


@pytest.mark.parametrize("ci", [3, 4])   # ("distmult", 4099, 7, 256, 129, 1) and ("complex", 777, 5, 512, 3, 0) of CASES
def test_random_table_counts_lie_inside_the_float64_intervals(ci):
    """The split kernel on the plain random inputs of test_fused_counts_equal_the_two_step_counts (true scores in the
    bulk of their rows, duplicate entity rows = exact ties, a hub row of filters), both tolerance pairs."""
    from kge_amd import engine as eng
    model, E, Rn, d, n, K, _ = CASES[ci]
    assert n <= 129
    rng = np.random.default_rng(E + 31 * n + K)
    T = _tables(eng, model, E, Rn, d, seed=E + n, flags=eng.FLAG_SPLIT_QUERY)
    s, p, o = (torch.from_numpy(rng.integers(0, hi, n)).to(DEV) for hi in (E, Rn, E))
    dup = rng.integers(0, E, min(E // 2, 40))
    T.ent[dup] = T.ent[rng.integers(0, E, len(dup))]
    t_sp, t_po = _true_scores(eng, T, s, p, o)
    f_sp = _filters(rng, n, E, K, o.cpu().numpy(), hub_rows=(n // 2,))
    f_po = _filters(rng, n, E, K, s.cpu().numpy(), hub_rows=(0,))
    sn, pn, on = (x.cpu().numpy() for x in (s, p, o))
    ent = T.ent.cpu()
    Q = R.split_queries64(model, ent, T.rel.cpu(), sn, pn, on)
    tab = R.table64(ent)
    for atol, rtol in ((1e-5, 1e-4), (0.05, 0.0)):
        cnt = _fused(eng, T, s, p, o, t_sp, t_po, f_sp, f_po, ((0, E),), atol, rtol).cpu().numpy()
        for si, (side, t, f, tc) in enumerate((("sp", t_sp, f_sp, on), ("po", t_po, f_po, sn))):
            fl = [tuple(x.cpu().numpy() for x in fs) for fs in f]
            b = R.count_bounds64(Q[side][0], Q[side][1], tab, t.cpu().numpy(), atol, rtol, model, fl, tc, 0)
            msg = (CASES[ci], atol, side, "undecided", int(b.und.sum()))
            assert (b.rank_min <= cnt[si, 0]).all() and (cnt[si, 0] <= b.rank_max).all(), msg
            assert (b.ties_min <= cnt[si, 1]).all() and (cnt[si, 1] <= b.ties_max).all(), msg
            print("RANDOM_CASE", *msg)


# ---- 3.4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [2, 1, 6, 9])   # one case per d and scorer
def test_a_bound_four_times_too_small_miscounts_the_planted_pairs(idx):
    """The band's table factor divided by four: pairs whose x_hi lies more than B / 4 outside the tie band are now
    counted from x_hi alone.  Rank and ties then differ from the split kernel's by what the reference predicts -- inside
    its interval on every row and ranking, and NOT zero on the rows with a discriminating pair (unless the reference
    itself sees a second pair that may cancel it).  Nothing is dropped: the lists only get shorter."""
    from kge_amd import engine as eng
    case, want, _, _, rep, t = _run(idx)
    T, s, p, o, f = _dev_inputs(eng, case)
    t_sp, t_po = (torch.from_numpy(t[side]).to(DEV) for side in SIDES)
    got, stats = _band_counts(eng, T, s, p, o, t_sp, t_po, f, case.chunks, case.K, scale=0.25)
    got = got.cpu().numpy()
    assert all(dropped == 0 for _, dropped in stats), stats
    msg = (R.PLANTED_CASES[idx], R.report_totals(case, rep), stats)
    for si, side in enumerate(SIDES):
        disc_rows = np.zeros(case.n, bool)
        iv = {}
        for comp, which in ((0, R.GREATER), (1, R.CLOSE)):
            lo_t = np.zeros((case.K + 1, case.n), np.int64)
            hi_t = np.zeros_like(lo_t)
            for c in range(len(case.chunks)):
                r = rep[side, c]
                lo, hi = R.scaled_band_diff(r.cp, r.bounds.masks, 0.25, which)
                lo_t += lo
                hi_t += hi
                disc_rows |= r.disc.any(1)
            diff = got[si, comp] - want[si, comp]
            bad = (diff < lo_t) | (diff > hi_t)
            assert not bad.any(), (msg, side, comp, np.argwhere(bad)[:5].tolist(), diff[bad][:5].tolist())
            iv[comp] = (lo_t, hi_t, diff)
        # the rows with a discriminating pair: their raw counts differ in the predicted component
        rows = np.nonzero(disc_rows)[0]
        assert len(rows) >= 1, msg
        seen = 0
        for i in rows:
            predicted = [comp for comp in (0, 1) if iv[comp][0][0, i] > 0 or iv[comp][1][0, i] < 0]
            for comp in predicted:
                assert iv[comp][2][0, i] != 0, (msg, side, int(i), comp)
            seen += bool(predicted)
        assert seen >= min(4, len(rows)), (msg, side, seen, len(rows))


# ---- 3.5 -------------------------------------------------------------------------------------------------------------
def _index(keys, vals, E):
    """FilterIndex's (keys, starts, values) arrays from (key, value) pairs."""
    kv = np.unique(keys * E + vals)
    k, v = kv // E, kv % E
    uk, start = np.unique(k, return_index=True)
    return tuple(torch.from_numpy(np.ascontiguousarray(x.astype(np.int64))).to(DEV)
                 for x in (uk, np.append(start, len(k)), v))


def test_eval_batch_band_equals_eval_batch_on_a_planted_batch():
    from kge_amd import engine as eng
    idx = 2   # ("distmult", 2111, 7, 256, 100, 2, one chunk)
    case = R.build_case(idx)
    assert (case.model, case.d, len(case.chunks), case.K) == ("distmult", 256, 1, 2)
    T, s, p, o, _ = _dev_inputs(eng, case)
    E, n, M = case.E, case.n, case.K + 1
    filters = []
    for k in range(case.K):
        pair = []
        for side, key in (("sp", case.s * case.R + case.p), ("po", case.p * E + case.o)):
            beg, end, vals = case.filters[side][k]
            cnt = end - beg
            rows = np.repeat(np.arange(n), cnt)
            v = np.concatenate([vals[b:e] for b, e in zip(beg, end)] + [np.zeros(0, np.int64)])
            pair.append(_index(key[rows], v, E))
        filters.append(tuple(pair))
    res = []
    for use_band in (False, True):
        band = eng.RankBand(T, n) if use_band else None
        counts = torch.zeros(2, 2, M, n, dtype=torch.int64, device=DEV)
        hist = torch.zeros(M, E, dtype=torch.float32, device=DEV)
        ro, rs = (torch.zeros(M, n, dtype=torch.int64, device=DEV) for _ in range(2))
        assert eng.eval_batch(T, s, p, o, filters, R.ATOL, R.RTOL, "rounded_mean_rank", counts, hist, ro, rs, band=band)
        if use_band:
            listed, dropped = band.status()
            assert dropped == 0 and listed >= 2 * n, (listed, dropped)
            assert int(band.list.view(torch.int32).view(-1, 1024)[:, 0].abs().sum()) == 0
        res.append(tuple(x.cpu() for x in (counts, hist, ro, rs)))
    for name, a, b in zip(("counts", "hist", "ranks_o", "ranks_s"), res[0], res[1]):
        assert torch.equal(a, b), (name, (a != b).nonzero()[:5].tolist())
