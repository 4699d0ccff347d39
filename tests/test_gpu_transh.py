"""The TransH kernels (csrc/transh.hip) through the C ABI on the GPU: every score and gradient within the derived bound of
tests/_transh_ref.py, and the placement-independence equalities bit for bit.  Tile edges of the pair kernel: 16 query
rows, 64 target rows, slices of 128 coordinates."""
import ctypes

import numpy as np
import pytest
import torch

import _transh_ref as th

pytestmark = pytest.mark.gpu

TQ, TT = 16, 64  # transh.hip: TH_TQ, TH_TT


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


def _pitched(x, ld, dev, misalign=False):
    """x [r, c] as a view with row pitch ld (> c) -- and, misaligned, one float off the 16-byte grid"""
    r, c = x.shape
    buf = torch.full((r * ld + 4,), float("nan"), device=dev)
    v = buf[1:1 + r * ld] if misalign else buf[:r * ld]
    v = v.view(r, ld)[:, :c]
    v.copy_(torch.from_numpy(x))
    return v


def _tables(ent, rel, lp, dev, layout="plain"):
    from kge_amd import engine
    if layout == "plain":
        e, r = torch.from_numpy(ent).to(dev), torch.from_numpy(rel).to(dev)
    elif layout == "pitched":  # a leading dimension larger than d, rows still 16-byte aligned where d % 4 == 0
        e, r = _pitched(ent, ent.shape[1] + 8, dev), _pitched(rel, rel.shape[1] + 4, dev)
    else:  # "element": an odd pitch and a base off the 16-byte grid: the element path
        e, r = _pitched(ent, ent.shape[1] + 3, dev, True), _pitched(rel, rel.shape[1] + 1, dev, True)
    return engine.Tables("transh", e, r, lp)


def _ix(x, dev, kind="i64"):
    t = torch.from_numpy(np.asarray(x)).to(dev)
    if kind == "i32":
        return t.int()
    if kind == "i64s2":  # stride 2
        buf = torch.full((2 * len(x),), -1, dtype=torch.int64, device=dev)
        buf[::2] = t
        return buf[::2]
    if kind == "i32s2":
        buf = torch.full((2 * len(x),), -1, dtype=torch.int32, device=dev)
        buf[::2] = t.int()
        return buf[::2]
    return t


def _case(d, n, E, seed):
    ent, rel = th.make_tables(E, 5, d, seed)
    rng = np.random.default_rng(seed + 100)
    # (relation 1 -- d_r = -EPS, w = 0 -- only in the planted triple: with it every pair (e, 1, e) has distance zero in
    # exact arithmetic and a rounding residue in float32, where the L2 gradient is not defined)
    s, p, o = rng.integers(0, E, n), rng.choice([0, 2, 3, 4], n), rng.integers(0, E, n)
    p[0] = 0  # w = 0
    if n > 2:
        s[2], p[2], o[2] = 0, 1, 0  # the zero-distance triple
    return ent, rel, s, p, o


def _within(got, want, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("d,n,m", [(1, 1, 1), (8, 3, TT - 1), (33, TQ + 1, TT), (128, 3, TT + 1), (136, TQ + 1, TT + 1)])
def test_scores_bound_and_placement_independence(dev, lp, d, n, m):
    from kge_amd import engine
    E = m
    ent, rel, s, p, o = _case(d, n, E, 11 * d + n)
    t = _tables(ent, rel, lp, dev)
    S, P, O = (_ix(x, dev) for x in (s, p, o))
    sp, po = engine.score_sp(t, S, P), engine.score_po(t, P, O)
    want, b = th.score_pairs(lp, "sp", ent, rel, s, p)
    _within(sp, want, b, "sp")
    want, b = th.score_pairs(lp, "po", ent, rel, o, p)
    _within(po, want, b, "po")
    # (iii) sp_po = sp next to po
    both = engine.score_sp_po(t, S, P, O)
    assert torch.equal(both[:, :m], sp) and torch.equal(both[:, m:], po)
    # (ii) spo and neg slot 2 = the sp column, neg slot 0 = spo on the expanded triples
    spo = engine.score_spo(t, S, P, O)
    ar = torch.arange(n, device=dev)
    assert torch.equal(spo, sp[ar, O])
    want, b = th.score_spo(lp, ent, rel, s, p, o)
    _within(spo, want, b, "spo")
    K = 5
    neg = torch.from_numpy(np.random.default_rng(d).integers(0, E, (n, K))).to(dev)
    n2 = engine.score_neg(t, S, P, O, 2, neg)
    assert torch.equal(n2, torch.gather(sp, 1, neg))
    n0 = engine.score_neg(t, S, P, O, 0, neg.int())
    exp = engine.score_spo(t, neg.reshape(-1), P.repeat_interleave(K), O.repeat_interleave(K)).view(n, K)
    assert torch.equal(n0, exp)
    want, b = th.score_neg(lp, ent, rel, s, p, o, 0, neg.cpu().numpy())
    _within(n0, want, b, "neg slot 0")
    # all / range / list, index types and strides, layouts: the same bits
    lo = min(1, m - 1)
    lst = np.array([m - 1, 0, 0, lo, m - 1])  # repeats
    for layout in ("plain", "pitched", "element"):
        t2 = _tables(ent, rel, lp, dev, layout)
        for kind in ("i32", "i64s2", "i32s2"):
            S2, P2, O2 = (_ix(x, dev, kind) for x in (s, p, o))
            assert torch.equal(engine.score_sp(t2, S2, P2), sp), (layout, kind)
            assert torch.equal(engine.score_po(t2, P2, O2), po), (layout, kind)
            assert torch.equal(engine.score_spo(t2, S2, P2, O2), spo), (layout, kind)
        assert torch.equal(engine.score_sp(t2, S, P, range(lo, m)), sp[:, lo:])
        assert torch.equal(engine.score_po(t2, P, O, range(lo, m)), po[:, lo:])
        L = _ix(lst, dev, "i32s2")
        assert torch.equal(engine.score_sp(t2, S, P, L), sp[:, lst])
        assert torch.equal(engine.score_sp_po(t2, S, P, O, L), torch.cat((sp[:, lst], po[:, lst]), 1))
        assert torch.equal(engine.score_neg(t2, S, P, O, 2, neg), n2)
        assert torch.equal(engine.score_neg(t2, S, P, O, 0, neg), n0)
    # ldo > m with canaries behind every row
    ldo = m + 3
    out = torch.full((n, ldo), 12345.0, device=dev)
    engine._pairs("kge_score_sp", t, S, P, None, None, out=out, ldo=ldo)
    assert torch.equal(out[:, :m], sp) and bool((out[:, m:] == 12345.0).all())
    out2 = torch.full((n, 2 * m + 3), 12345.0, device=dev)
    from kge_amd import _lib
    keep = []
    si, pi, oi = (engine._index(x, dev, keep) for x in (S, P, O))
    ti, _ = engine._targets(None, t, keep)
    tc = t.c()
    rc = _lib.lib().kge_score_sp_po(ctypes.byref(tc), si, pi, oi, n, ti, m, out2.data_ptr(), 2 * m + 3, None, 0,
                                    engine._stream_handle(dev))
    assert rc == 0
    assert torch.equal(out2[:, :m], sp) and torch.equal(out2[:, m:2 * m], po) and bool((out2[:, 2 * m:] == 12345.0).all())


@pytest.mark.parametrize("lp", [1.0, 2.0])
def test_zero_normal_is_the_shifted_transe_distance(dev, lp):
    from kge_amd import engine
    d, E = 33, 20
    ent, rel = th.make_tables(E, 3, d, 4)
    rel[:, d:] = 0.0
    s, p = np.arange(5), np.array([0, 2, 2, 0, 2])
    t = _tables(ent, rel, lp, dev)
    got = engine.score_sp(t, _ix(s, dev), _ix(p, dev))
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    v = (e64[s] + r64[p][:, :d])[:, None, :] - e64[None, :, :] + th.EPS
    want = -np.abs(v).sum(2) if lp == 1.0 else -np.sqrt((v * v).sum(2))
    _, b = th.score_pairs(lp, "sp", ent, rel, s, p)
    _within(got, want, b, "zero w")


@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("d,n,m", [(1, 1, 1), (8, 3, 7), (33, TQ + 1, TT + 1), (128, 3, 5), (136, 2, 3)])
def test_backward_entries_within_the_bound(dev, lp, d, n, m):
    from kge_amd import engine
    E = max(m, 6)
    ent, rel, s, p, o = _case(d, n, E, 7 * d + m)
    rng = np.random.default_rng(d + m)
    t = _tables(ent, rel, lp, dev)
    S, P, O = (_ix(x, dev, "i32s2") for x in (s, p, o))
    for direction, a, A in (("sp", s, S), ("po", o, O)):
        for targets in (None, np.array([E - 1, 0, 0, min(1, E - 1)])):
            mm = E if targets is None else len(targets)
            G = rng.standard_normal((n, mm)).astype(np.float32)
            (w_a, w_p, w_t), (b_a, b_p, b_t), safe = th.pairs_bwd(lp, direction, ent, rel, a, p, targets, G)
            assert safe
            tg = None if targets is None else _ix(targets, dev)
            g1 = engine.score_pairs_bwd(t, direction, A, P, tg, torch.from_numpy(G).to(dev))
            g2 = engine.score_pairs_bwd(t, direction, A, P, tg, torch.from_numpy(G).to(dev))
            for x, y in zip(g1, g2):  # (vii) no atomics
                assert torch.equal(x, y)
            _within(g1[0], w_a, b_a, "g_a")
            _within(g1[1], w_p, b_p, "g_p")
            _within(g1[2], w_t, b_t, "g_tgt")
    # spo_bwd rows, spo_bwd_accum and neg_bwd_accum on PRELOADED gradients
    g = rng.standard_normal(n).astype(np.float32)
    (w_s, w_p, w_o), (b_s, b_p, b_o), safe = th.spo_bwd(lp, ent, rel, s, p, o, g)
    assert safe
    g_s, g_p, g_o = engine.score_spo_bwd(t, S, P, O, torch.from_numpy(g).to(dev))
    _within(g_s, w_s, b_s, "g_s")
    _within(g_p, w_p, b_p, "g_p")
    _within(g_o, w_o, b_o, "g_o")
    pre_e = rng.standard_normal(ent.shape).astype(np.float32)
    pre_r = rng.standard_normal(rel.shape).astype(np.float32)
    U = th.U
    (w_e, w_r), (b_e, b_r), _ = th.neg_bwd_accum(lp, ent, rel, s, p, o, 2, o[:, None], g[:, None])
    ge, gr = torch.from_numpy(pre_e).to(dev), torch.from_numpy(pre_r).to(dev)
    assert engine.score_spo_bwd_accum(t, S, P, O, torch.from_numpy(g).to(dev), None, ge, gr)
    # the preloaded value joins the atomic sum: one more term per element
    _within(ge, w_e + pre_e, b_e + 2 * U * (np.abs(w_e) + np.abs(pre_e) + b_e), "accum ent")
    _within(gr, w_r + pre_r, b_r + 2 * U * (np.abs(w_r) + np.abs(pre_r) + b_r), "accum rel")
    K = 35  # more than one chunk of 32 negatives
    neg = rng.integers(0, E, (n, K))
    if n > 2:
        neg[2, 0] = 0
    G = rng.standard_normal((n, K)).astype(np.float32)
    for slot in (0, 2):
        (w_e, w_r), (b_e, b_r), safe = th.neg_bwd_accum(lp, ent, rel, s, p, o, slot, neg, G)
        assert safe
        ge, gr = torch.from_numpy(pre_e).to(dev), torch.from_numpy(pre_r).to(dev)
        assert engine.score_neg_bwd_accum(t, S, P, O, slot, _ix(neg, dev), torch.from_numpy(G).to(dev), None, ge, gr)
        # a positive's own rows arrive as ceil(K / 32) partial sums: the same terms in another grouping
        _within(ge, w_e + pre_e, b_e + 3 * U * (np.abs(w_e) + np.abs(pre_e) + b_e), f"neg accum ent {slot}")
        _within(gr, w_r + pre_r, b_r + 3 * U * (np.abs(w_r) + np.abs(pre_r) + b_r), f"neg accum rel {slot}")


def test_empty_sides(dev):
    from kge_amd import engine
    ent, rel, s, p, o = _case(8, 3, 10, 1)
    t = _tables(ent, rel, 1.0, dev)
    S, P = _ix(s, dev), _ix(p, dev)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    assert tuple(engine.score_sp(t, none, none).shape) == (0, 10)
    assert tuple(engine.score_sp(t, S, P, none).shape) == (3, 0)
    # m == 0 (a target list of which no element is used): g_a = g_p = 0, g_tgt untouched
    from kge_amd import _lib
    keep = []
    si, pi = engine._index(S, dev, keep), engine._index(P, dev, keep)
    g_a, g_p = torch.full((3, 8), 7.0, device=dev), torch.full((3, 16), 7.0, device=dev)
    g_t, gout = torch.full((4,), 7.0, device=dev), torch.ones(3, 4, device=dev)
    tc = t.c()
    rc = _lib.lib().kge_score_pairs_bwd(ctypes.byref(tc), _lib.SP_, si, pi, 3, si, 0, gout.data_ptr(), 4, None, 0,
                                        g_a.data_ptr(), g_p.data_ptr(), g_t.data_ptr(), None, 0, engine._stream_handle(dev))
    assert rc == 0
    assert not g_a.any() and not g_p.any() and bool((g_t == 7.0).all())
    # n == 0 against all 10 entities: g_tgt = 0, g_a / g_p untouched
    g_a.fill_(7.0), g_p.fill_(7.0)
    g_t = torch.full((10, 8), 7.0, device=dev)
    ti, m = engine._targets(None, t, keep)
    rc = _lib.lib().kge_score_pairs_bwd(ctypes.byref(tc), _lib.PO_, si, pi, 0, ti, m, gout.data_ptr(), 10, None, 0,
                                        g_a.data_ptr(), g_p.data_ptr(), g_t.data_ptr(), None, 0, engine._stream_handle(dev))
    assert rc == 0 and m == 10
    assert not g_t.any() and bool((g_a == 7.0).all()) and bool((g_p == 7.0).all())


def test_score_matrix_is_all_the_entry_needs(dev):
    """E = 2,000, n = 64, d = 64: the reference's form would hold [m, n, d] (33 MB); the entry writes [n, m]."""
    from kge_amd import engine
    ent, rel = th.make_tables(2000, 7, 64, 9)
    rng = np.random.default_rng(1)
    s, p = rng.integers(0, 2000, 64), rng.integers(0, 7, 64)
    t = _tables(ent, rel, 2.0, dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    got = engine.score_sp(t, _ix(s, dev), _ix(p, dev))
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(dev) - base < 4 * 64 * 2000 * 4  # a few score matrices at most, not n m d
    want, b = th.score_pairs(2.0, "sp", ent, rel, s, p)
    _within(got, want, b, "sp 2000")


@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("d,E", [(8, 16385), (128, 4097), (136, 4097)])
def test_many_target_tiles_per_workgroup_give_the_same_bits(dev, lp, d, E):
    """n = 512 query rows: the launch gives a workgroup 8 (E = 16385) or 2 (E = 4097) target tiles, and for d <= 128 the
    query tile stays in LDS across them.  The bits must be those of the same rows scored 16 at a time (one tile per
    workgroup) and of kge_score_spo."""
    from kge_amd import engine
    n = 512
    ent, rel = th.make_tables(E, 5, d, d + E)
    rng = np.random.default_rng(E)
    s, p, o = rng.integers(0, E, n), rng.integers(0, 5, n), rng.integers(0, E, n)
    t = _tables(ent, rel, lp, dev)
    S, P, O = (_ix(x, dev) for x in (s, p, o))
    sp, po = engine.score_sp(t, S, P, padded=False), engine.score_po(t, P, O, padded=False)
    for i in range(0, n, TQ):
        assert torch.equal(engine.score_sp(t, S[i:i + TQ], P[i:i + TQ]), sp[i:i + TQ]), i
        assert torch.equal(engine.score_po(t, P[i:i + TQ], O[i:i + TQ]), po[i:i + TQ]), i
    ar = torch.arange(n, device=dev)
    assert torch.equal(engine.score_spo(t, S, P, O), sp[ar, O])
    both = engine.score_sp_po(t, S, P, O)
    assert torch.equal(both[:, :E], sp) and torch.equal(both[:, E:], po)
    rows = np.array([0, 17, 511])
    want, b = th.score_pairs(lp, "sp", ent, rel, s[rows], p[rows])
    _within(sp[rows], want, b, "sp")


@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("d,n,K", [(33, 3, 40), (8, 2, 300), (128, 5, 700)])
def test_score_neg_with_long_runs_of_negatives(dev, lp, d, n, K):
    """K = 40: a group of the launch takes a second negative; K = 300, 700: more than one workgroup per positive."""
    from kge_amd import engine
    E = 50
    ent, rel, s, p, o = _case(d, n, E, d + K)
    t = _tables(ent, rel, lp, dev)
    S, P, O = (_ix(x, dev) for x in (s, p, o))
    neg = torch.from_numpy(np.random.default_rng(K).integers(0, E, (n, K))).to(dev)
    sp = engine.score_sp(t, S, P)
    n2 = engine.score_neg(t, S, P, O, 2, neg)
    assert torch.equal(n2, torch.gather(sp, 1, neg))
    n0 = engine.score_neg(t, S, P, O, 0, neg)
    exp = engine.score_spo(t, neg.reshape(-1), P.repeat_interleave(K), O.repeat_interleave(K)).view(n, K)
    assert torch.equal(n0, exp)
    want, b = th.score_neg(lp, ent, rel, s, p, o, 0, neg.cpu().numpy())
    _within(n0, want, b, "neg slot 0")
