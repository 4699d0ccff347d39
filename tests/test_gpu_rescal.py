"""The RESCAL kernels (csrc/rescal.hip) through the C ABI on the GPU: every score and gradient within the derived bound of
tests/_rescal_ref.py, and the equalities between entry points bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import _rescal_ref as rr

pytestmark = pytest.mark.gpu

VW, SLICE = 4, 32        # rescal_device.hpp: a group of four columns, the stride of a partial sum's groups
ROWS = 32                # rs_matvec: rows of M per pass of a workgroup (RS_THREADS / 8)
CHUNK8 = 8               # rs_row_dot: a lane's chunk (score_spo.hip's)
BM, BN = 128, 128        # score_pairs_f32.hip: F3_BM x F3_BN, the tile of the second stage
NEG_CHUNK = 256          # rescal.hip: RS_NEG_CHUNK
# d: 1; one chunk; an odd width (element path) above one slice; a multiple of everything; % 8 == 0 but past 128; % 4 == 0
# but % 8 != 0 (vector build, element dots); the limit
SHAPES = [(1, 1, 1), (8, 3, BN - 1), (33, BM + 1, BN), (128, 3, BN + 1), (136, ROWS + 1, BN + 1), (12, BM - 1, 5),
          (8, BM, 5), (256, 2, 7)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


def _pitched(x, ld, dev, misalign=False):
    """x [r, c] as a view with row pitch ld (> c) in a NaN-filled buffer -- and, misaligned, one float off the 16-byte grid"""
    r, c = x.shape
    buf = torch.full((r * ld + 4,), float("nan"), device=dev)
    v = buf[1:1 + r * ld] if misalign else buf[:r * ld]
    v = v.view(r, ld)[:, :c]
    v.copy_(torch.from_numpy(x))
    return v


def _tables(ent, rel, dev, layout="plain", flags=0):
    from kge_amd import engine
    if layout == "plain":
        e, r = torch.from_numpy(ent).to(dev), torch.from_numpy(rel).to(dev)
    elif layout == "pitched":
        e, r = _pitched(ent, ent.shape[1] + 8, dev), _pitched(rel, rel.shape[1] + 4, dev)
    else:  # "element": an odd pitch and a base off the 16-byte grid
        e, r = _pitched(ent, ent.shape[1] + 3, dev, True), _pitched(rel, rel.shape[1] + 1, dev, True)
    return engine.Tables("rescal", e, r, 1.0, flags)


def _ix(x, dev, kind="i64"):
    t = torch.from_numpy(np.asarray(x)).to(dev)
    if kind == "i32":
        return t.int()
    if kind == "i64s2":
        buf = torch.full((2 * len(x),), -1, dtype=torch.int64, device=dev)
        buf[::2] = t
        return buf[::2]
    if kind == "i32s2":
        buf = torch.full((2 * len(x),), -1, dtype=torch.int32, device=dev)
        buf[::2] = t.int()
        return buf[::2]
    return t


def _case(d, n, E, seed):
    ent, rel = rr.make_tables(E, 5, d, seed)
    rng = np.random.default_rng(seed + 100)
    s, p, o = rng.integers(0, E, n), rng.integers(0, 5, n), rng.integers(0, E, n)
    p[0] = 1  # the zero matrix
    if n > 1:
        p[1] = 2  # the identity
    if n > 2:
        p[2], s[2] = p[0], s[0]  # a repeated relation and a repeated entity
    return ent, rel, s, p, o


def _within(got, ref, what):
    want, e = ref
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), what
    err, b = np.abs(got - want), rr.bound(e)
    assert (err <= b).all(), (what, float((err / b).max()))


@pytest.mark.parametrize("d,n,m", SHAPES)
def test_scores_bound_and_bit_equalities(dev, d, n, m):
    from kge_amd import engine
    E = m
    ent, rel, s, p, o = _case(d, n, E, 11 * d + n)
    t = _tables(ent, rel, dev)
    S, P, O = (_ix(x, dev) for x in (s, p, o))
    sp, po = engine.score_sp(t, S, P), engine.score_po(t, P, O)
    _within(sp, rr.score_pairs("sp_", ent, rel, s, p), "sp")
    _within(po, rr.score_pairs("_po", ent, rel, o, p), "po")
    # the two stages: kge_rescal_queries, then DistMult on (q, ones, targets)
    q_sp, q_po = engine.rescal_queries(t, "sp_", S, P), engine.rescal_queries(t, "_po", O, P)
    _within(q_sp, rr.queries("sp_", ent, rel, s, p), "q sp_")
    _within(q_po, rr.queries("_po", ent, rel, o, p), "q _po")
    ones = torch.ones(n, d, device=dev)
    assert torch.equal(engine.score_emb("distmult", q_sp, ones, t.ent, "sp_"), sp)
    assert torch.equal(engine.score_emb("distmult", t.ent, ones, q_po, "_po"), po)
    both = engine.score_sp_po(t, S, P, O)
    assert torch.equal(both[:, :m], sp) and torch.equal(both[:, m:], po)
    tn = _tables(ent, rel, dev, flags=engine.FLAG_NO_MFMA)
    assert torch.equal(engine.score_sp(tn, S, P), sp) and torch.equal(engine.score_po(tn, P, O), po)
    assert torch.equal(engine.score_sp_po(tn, S, P, O), both)
    # row-wise: spo, neg
    spo = engine.score_spo(t, S, P, O)
    _within(spo, rr.score_spo(ent, rel, s, p, o), "spo")
    assert torch.equal(spo, engine.score_emb("distmult", q_sp, ones, t.ent[O], "spo").view(-1))
    K = 5
    negn = np.random.default_rng(d).integers(0, E, (n, K))
    neg = torch.from_numpy(negn).to(dev)
    n2 = engine.score_neg(t, S, P, O, 2, neg)
    exp = engine.score_spo(t, S.repeat_interleave(K), P.repeat_interleave(K), neg.reshape(-1)).view(n, K)
    assert torch.equal(n2, exp)
    _within(n2, rr.score_neg(ent, rel, s, p, o, 2, negn), "neg slot 2")
    n0 = engine.score_neg(t, S, P, O, 0, neg.int())
    _within(n0, rr.score_neg(ent, rel, s, p, o, 0, negn), "neg slot 0")
    exp0 = engine.score_emb("distmult", q_po.repeat_interleave(K, 0), ones.repeat_interleave(K, 0), t.ent[neg.reshape(-1)],
                            "spo").view(n, K)
    assert torch.equal(n0, exp0)
    # all / range / list targets, index types and strides, layouts: the same bits
    lo = min(1, m - 1)
    lst = np.array([m - 1, 0, 0, lo, m - 1])
    for layout in ("plain", "pitched", "element"):
        t2 = _tables(ent, rel, dev, layout)
        for kind in ("i32", "i64s2", "i32s2"):
            S2, P2, O2 = (_ix(x, dev, kind) for x in (s, p, o))
            assert torch.equal(engine.score_sp(t2, S2, P2), sp), (layout, kind)
            assert torch.equal(engine.score_po(t2, P2, O2), po), (layout, kind)
            assert torch.equal(engine.score_spo(t2, S2, P2, O2), spo), (layout, kind)
            assert torch.equal(engine.rescal_queries(t2, "sp_", S2, P2), q_sp), (layout, kind)
            assert torch.equal(engine.rescal_queries(t2, "_po", O2, P2), q_po), (layout, kind)
        assert torch.equal(engine.score_sp(t2, S, P, range(lo, m)), sp[:, lo:])
        assert torch.equal(engine.score_po(t2, P, O, _ix(lst, dev, "i32")), po[:, lst])
        assert torch.equal(engine.score_sp_po(t2, S, P, O, _ix(lst, dev)), torch.cat([sp[:, lst], po[:, lst]], 1))
        assert torch.equal(engine.score_neg(t2, S, P, O, 2, neg), n2) and torch.equal(engine.score_neg(t2, S, P, O, 0, neg), n0)


def test_queries_do_not_depend_on_n_or_row_position(dev):
    from kge_amd import engine
    d, E = 33, 9
    ent, rel, s, p, o = _case(d, 40, E, 5)
    t = _tables(ent, rel, dev)
    S, P = _ix(s, dev), _ix(p, dev)
    full = engine.rescal_queries(t, "sp_", S, P)
    perm = torch.randperm(40, device=dev)
    assert torch.equal(engine.rescal_queries(t, "sp_", S[perm], P[perm]), full[perm])
    assert torch.equal(engine.rescal_queries(t, "sp_", S[7:8], P[7:8]), full[7:8])
    wide = torch.full((40, d + 5), float("nan"), device=dev)
    engine.rescal_queries(t, "_po", S, P, out=wide[:, :d])
    assert torch.equal(wide[:, :d], engine.rescal_queries(t, "_po", S, P)) and torch.isnan(wide[:, d:]).all()


@pytest.mark.parametrize("d,n,m", [(1, 1, 1), (8, 3, 5), (33, ROWS + 1, BN + 1), (136, 3, 9), (256, 2, 3)])
@pytest.mark.parametrize("layout", ["plain", "element"])
def test_gradients(dev, d, n, m, layout):
    from kge_amd import engine
    E = m
    ent, rel, s, p, o = _case(d, n, E, 7 * d + n)
    t = _tables(ent, rel, dev, layout)
    S, P, O = (_ix(x, dev, "i32") for x in (s, p, o))
    rng = np.random.default_rng(d + n)
    lst = rng.integers(0, E, 4)
    for direction, a, A in (("sp_", s, S), ("_po", o, O)):
        for targets, T in ((None, None), (lst, _ix(lst, dev))):
            mm = E if targets is None else len(lst)
            g = rng.standard_normal((n, mm)).astype(np.float32)
            G = torch.from_numpy(g).to(dev)
            got = engine.score_pairs_bwd(t, "sp" if direction == "sp_" else "po", A, P, T, G)
            again = engine.score_pairs_bwd(t, "sp" if direction == "sp_" else "po", A, P, T, G)
            want = rr.pairs_bwd(direction, ent, rel, a, p, targets, g)
            for x, y, w, name in zip(got, again, want, ("g_a", "g_p", "g_tgt")):
                _within(x, w, (direction, name))
                assert torch.equal(x, y), (direction, name)  # no float atomics
    # spo: per-row outputs, then the same accumulated into table gradients
    g = rng.standard_normal(n).astype(np.float32)
    G = torch.from_numpy(g).to(dev)
    gs, gp, go = engine.score_spo_bwd(t, S, P, O, G)
    (wa, wm, wx) = rr.rows_bwd("sp_", ent, rel, s, p, o[:, None], g[:, None])
    _within(gs, wa, "spo g_s"); _within(gp, wm, "spo g_p"); _within(go, (wx[0][:, 0], wx[1][:, 0]), "spo g_o")
    ge, gr = torch.zeros(E, d, device=dev), torch.zeros(5, d * d, device=dev)
    assert engine.score_spo_bwd_accum(t, S, P, O, G, None, ge, gr)
    _within(ge, rr.accum([(s, *wa), (o, wx[0][:, 0], wx[1][:, 0])], (E, d)), "spo accum ent")
    _within(gr, rr.accum([(p, *wm)], (5, d * d)), "spo accum rel")
    # neg, both slots
    K = 3
    negn = rng.integers(0, E, (n, K))
    negn[0, 1] = negn[0, 0]  # a repeated sample
    g = rng.standard_normal((n, K)).astype(np.float32)
    for slot, direction, a in ((2, "sp_", s), (0, "_po", o)):
        ge, gr = torch.zeros(E, d, device=dev), torch.zeros(5, d * d, device=dev)
        assert engine.score_neg_bwd_accum(t, S, P, O, slot, torch.from_numpy(negn).to(dev), torch.from_numpy(g).to(dev),
                                          None, ge, gr)
        wa, wm, wx = rr.rows_bwd(direction, ent, rel, a, p, negn, g)
        _within(ge, rr.accum([(a, *wa), (negn, wx[0].reshape(-1, d), wx[1].reshape(-1, d))], (E, d)), ("neg ent", slot))
        _within(gr, rr.accum([(p, *wm)], (5, d * d)), ("neg rel", slot))


def test_neg_backward_across_the_register_chunk(dev):
    from kge_amd import engine
    d, n, E, K = 12, 2, 7, NEG_CHUNK + 1
    ent, rel, s, p, o = _case(d, n, E, 3)
    t = _tables(ent, rel, dev)
    S, P, O = (_ix(x, dev) for x in (s, p, o))
    rng = np.random.default_rng(0)
    negn, g = rng.integers(0, E, (n, K)), rng.standard_normal((n, K)).astype(np.float32)
    for slot, direction, a in ((2, "sp_", s), (0, "_po", o)):
        ge, gr = torch.zeros(E, d, device=dev), torch.zeros(5, d * d, device=dev)
        assert engine.score_neg_bwd_accum(t, S, P, O, slot, torch.from_numpy(negn).to(dev), torch.from_numpy(g).to(dev),
                                          None, ge, gr)
        # the two chunks of a positive arrive as two atomic contributions: the reference takes them as two rows
        parts_e, parts_r = [], []
        for lo, hi in ((0, NEG_CHUNK), (NEG_CHUNK, K)):
            wa, wm, wx = rr.rows_bwd(direction, ent, rel, a, p, negn[:, lo:hi], g[:, lo:hi])
            parts_e += [(a, *wa), (negn[:, lo:hi], wx[0].reshape(-1, d), wx[1].reshape(-1, d))]
            parts_r += [(p, *wm)]
        _within(ge, rr.accum(parts_e, (E, d)), ("ent", slot))
        _within(gr, rr.accum(parts_r, (5, d * d)), ("rel", slot))
        _within(engine.score_neg(t, S, P, O, slot, torch.from_numpy(negn).to(dev)),
                rr.score_neg(ent, rel, s, p, o, slot, negn), ("scores", slot))


def test_empty_sides_and_workspace(dev):
    from kge_amd import _lib, engine
    d, E = 8, 6
    ent, rel, s, p, o = _case(d, 3, E, 1)
    t = _tables(ent, rel, dev)
    S, P, O = (_ix(x, dev) for x in (s, p, o))
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    assert tuple(engine.score_sp(t, none, none).shape) == (0, E)
    assert tuple(engine.score_sp(t, S, P, none).shape) == (3, 0)
    assert tuple(engine.score_spo(t, none, none, none).shape) == (0,)
    assert tuple(engine.rescal_queries(t, "sp_", none, none).shape) == (0, d)
    # kge_score_pairs_bwd: an empty side zeroes the other side's gradients (the entry's convention)
    # a missing workspace
    tc = t.c()
    out = torch.empty(3, E, device=dev)
    ix = lambda x: _lib.KgeIndex(x.data_ptr(), 1, 0, 1)
    tg = _lib.KgeIndex(None, 1, 0, 1)
    L = _lib.lib()
    need = L.kge_score_workspace_bytes(ctypes.byref(tc), 3)
    assert need == 4 * (2 * 3 * d + d) and L.kge_rescal_queries_bytes(ctypes.byref(tc), 3) == 4 * 3 * d
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert L.kge_score_sp(ctypes.byref(tc), ix(S), ix(P), 3, tg, E, out.data_ptr(), E, None, 0, None) == -5
    assert L.kge_score_sp(ctypes.byref(tc), ix(S), ix(P), 3, tg, E, out.data_ptr(), E, ws.data_ptr(), 16, None) == -5
    half = 4 * (3 * d + d)
    assert L.kge_score_sp(ctypes.byref(tc), ix(S), ix(P), 3, tg, E, out.data_ptr(), E, ws.data_ptr(), half, None) == 0
    out2 = torch.empty(3, 2 * E, device=dev)
    assert L.kge_score_sp_po(ctypes.byref(tc), ix(S), ix(P), ix(O), 3, tg, E, out2.data_ptr(), 2 * E, ws.data_ptr(), half,
                             None) == -5
    # kge_score_pairs_bwd without targets (a list of none): g_a and g_p are overwritten with zeros, no workspace needed
    ga, gp = torch.full((3, d), float("nan"), device=dev), torch.full((3, d * d), float("nan"), device=dev)
    assert L.kge_score_pairs_bwd(ctypes.byref(tc), 1, ix(S), ix(P), 3, ix(S), 0, out.data_ptr(), 1, None, 0, ga.data_ptr(),
                                 gp.data_ptr(), out.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert not ga.any() and not gp.any()
    # n == 0 / num_neg == 0: kge_score_neg and the _accum entries accept it and touch nothing
    ge, gr = torch.full((E, d), 7.0, device=dev), torch.full((5, d * d), 7.0, device=dev)
    for nn, K in ((0, 4), (3, 0)):
        assert L.kge_score_neg(ctypes.byref(tc), ix(S), ix(P), ix(O), nn, 2, S.data_ptr(), 1, 4, K, out.data_ptr(), 4, None) == 0
        assert L.kge_score_neg_bwd_accum(ctypes.byref(tc), ix(S), ix(P), ix(O), nn, 0, S.data_ptr(), 1, 4, K, out.data_ptr(), 4,
                                         None, 0, ge.data_ptr(), d, gr.data_ptr(), d * d, None) == 0
    assert L.kge_score_spo_bwd_accum(ctypes.byref(tc), ix(S), ix(P), ix(O), 0, out.data_ptr(), None, ge.data_ptr(), d,
                                     gr.data_ptr(), d * d, None) == 0
    assert L.kge_score_spo_bwd(ctypes.byref(tc), ix(S), ix(P), ix(O), 0, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((ge == 7.0).all()) and bool((gr == 7.0).all())
    # kge_score_pairs_bwd without queries: g_tgt is overwritten with zeros (the entry's convention), no workspace needed
    gt = torch.full((E, d), float("nan"), device=dev)
    assert L.kge_score_pairs_bwd(ctypes.byref(tc), 1, ix(S), ix(P), 0, tg, E, out.data_ptr(), E, None, 0, out.data_ptr(),
                                 out.data_ptr(), gt.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert not gt.any()
    assert torch.equal(out, engine.score_sp(t, S, P))
