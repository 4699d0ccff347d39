"""The relation-grouped RESCAL route (csrc/rescal_grouped.hip) on the GPU against the float64 reference of
tests/_rescal_ref.py: every comparison is |got - float64| <= the bound the reference returns for that element (its
(K - 1) u sum |x_k| rule holds for a K-term sum in any order: it covers the MFMA chains, the plain adds and the atomics).
One sweep per axis around a base case (d = 33, n = 70 on a random draw, 3 samples, slot 2, int64 indexes, plain tables).
The pattern "sizes" holds groups of exactly 16, 17, 32 and 33 rows beside empty relations: 98 rows, not 70."""
import numpy as np
import pytest
import torch

import _rescal_ref as rr
import _tucker3_ref as tr

pytestmark = pytest.mark.gpu

E, R = 40, 9
DIMS = (1, 15, 16, 17, 33, 100, 256)          # padded k and column edges, no multiple of 4, the panelled M_p
PATTERNS = ("random", "one", "own", "sizes")
BASE = dict(d=33, pattern="random", K=3, slot=2, kind="i64", layout="plain")
SWEEP = ([dict(BASE, d=d) for d in DIMS] + [dict(BASE, pattern=x) for x in PATTERNS[1:]] +
         [dict(BASE, K=1), dict(BASE, K=257), dict(BASE, slot=0), dict(BASE, slot=0, d=100), dict(BASE, kind="i32"),
          dict(BASE, kind="i64s2"), dict(BASE, layout="pitched")])
_ID = lambda c: "-".join(str(v) for v in c.values())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


def _relations(pattern):
    rng = np.random.default_rng(5)
    if pattern == "one":       # several row tiles of one group
        return np.full(70, 3)
    if pattern == "own":       # every row on its own relation
        return rng.permutation(R)
    if pattern == "sizes":     # relations 0, 4, 6, 7, 8 stay empty
        return rng.permutation(np.repeat([1, 2, 3, 5], [16, 17, 32, 33]))
    return rng.integers(0, R, 70)


def _pitched(x, pad, dev):
    """x [r, c] as a view on the row pitch c + pad of a NaN-filled buffer: the guard words stay NaN"""
    r, c = x.shape
    buf = torch.full((r, c + pad), float("nan"), device=dev)
    buf[:, :c] = torch.from_numpy(x)
    return buf[:, :c]


def _guards_intact(v):
    return bool(torch.isnan(v._base[:, v.shape[1]:]).all())


def _ix(x, dev, kind):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if kind == "i32":
        return t.int()
    if kind == "i64s2":
        buf = torch.full((2 * len(x),), -1, dtype=torch.int64, device=dev)
        buf[::2] = t
        return buf[::2]
    return t


def _case(c, dev):
    from kge_amd import engine
    ent, rel = rr.make_tables(E, R, c["d"], 7)
    p = _relations(c["pattern"])
    rng = np.random.default_rng(len(p) + c["d"])
    s, o = rng.integers(0, E, len(p)), rng.integers(0, E, len(p))
    s[1], o[1] = s[0], o[0]  # a repeated entity
    if c["layout"] == "pitched":
        t = engine.Tables("rescal", _pitched(ent, 8, dev), _pitched(rel, 4, dev))
    else:
        t = engine.Tables("rescal", torch.from_numpy(ent).to(dev), torch.from_numpy(rel).to(dev))
    return t, ent, rel, s, p, o, [_ix(x, dev, c["kind"]) for x in (s, p, o)]


def _within(got, ref, what):
    want, e = ref
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    ratio = np.abs(got - want) / rr.bound(e)
    print("err/bound", what, float(ratio.max()))
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), (what, float(ratio.max()))


@pytest.mark.parametrize("pattern,kind", [(x, "i64") for x in PATTERNS] + [("random", "i32"), ("random", "i64s2")])
def test_grouping_is_the_stable_sort(dev, pattern, kind):
    from kge_amd import engine
    t, ent, rel, s, p, o, (S, P, O) = _case(dict(BASE, pattern=pattern, kind=kind, d=4), dev)
    perm, G, group_rel, group_begin = (x.cpu().numpy() for x in engine.rescal_group(t, P))
    ids, first = np.unique(np.sort(p, kind="stable"), return_index=True)
    g = int(G[0])
    assert g == len(ids)
    assert np.array_equal(perm, np.argsort(p, kind="stable"))
    assert np.array_equal(group_rel[:g], ids) and np.array_equal(group_begin[:g + 1], np.append(first, len(p)))


@pytest.mark.parametrize("c", [x for x in SWEEP if x["K"] == 3], ids=_ID)
def test_queries_inside_the_bound(dev, c):
    from kge_amd import engine
    t, ent, rel, s, p, o, (S, P, O) = _case(c, dev)
    direction, a, A = ("sp_", s, S) if c["slot"] == 2 else ("_po", o, O)
    out = _pitched(np.zeros((len(p), c["d"]), np.float32), 5, dev)
    q = engine.rescal_queries(t, direction, A, P, out=out, grouped=True)
    _within(q, rr.queries(direction, ent, rel, a, p), ("q", direction))
    assert _guards_intact(out) and (c["layout"] == "plain" or (_guards_intact(t.ent) and _guards_intact(t.rel)))
    # not the REDUCE8 chain of kge_rescal_queries -- the same real number: inside the sum of the two bounds
    plain = engine.rescal_queries(t, direction, A, P)
    e = rr.queries(direction, ent, rel, a, p)[1]
    assert ((q - plain).abs().cpu().numpy() <= 2 * rr.bound(e)).all()


@pytest.mark.parametrize("direction", ["sp_", "_po"])
def test_a_query_row_is_a_pure_function_of_its_two_rows(dev, direction):
    """the same (entity, relation) pair at other batch positions, among other group-mates and in a batch of another n"""
    from kge_amd import engine
    t, ent, rel, s, p, o, _ = _case(dict(BASE, d=100), dev)
    a, n = s, len(p)
    q = engine.rescal_queries(t, direction, _ix(a, dev, "i64"), _ix(p, dev, "i64"), grouped=True)
    rng = np.random.default_rng(2)
    shuffle = rng.permutation(n)
    q2 = engine.rescal_queries(t, direction, _ix(a[shuffle], dev, "i32"), _ix(p[shuffle], dev, "i32"), grouped=True)
    assert torch.equal(q2, q[torch.from_numpy(shuffle).to(dev)])
    # 23 of the rows, every one now beside rows of ONE other relation pattern: all relations but its own set to its own
    pick = shuffle[:23]
    a3, p3 = np.concatenate([a[pick], a[:17]]), np.concatenate([p[pick], np.full(17, p[pick[0]])])
    q3 = engine.rescal_queries(t, direction, _ix(a3, dev, "i64s2"), _ix(p3, dev, "i64"), grouped=True)
    assert torch.equal(q3[:23], q[torch.from_numpy(pick).to(dev)])


def _backward(t, S, P, O, slot, neg, g, ge0, gr0, dev, pitched):
    from kge_amd import engine
    ge = _pitched(ge0, 3, dev) if pitched else torch.from_numpy(ge0).to(dev)
    gr = _pitched(gr0, 5, dev) if pitched else torch.from_numpy(gr0).to(dev)
    assert engine.score_neg_bwd_accum_grouped(t, S, P, O, slot, neg, g, None, ge, gr)
    assert not pitched or (_guards_intact(ge) and _guards_intact(gr))
    return ge, gr


@pytest.mark.parametrize("c", SWEEP, ids=_ID)
def test_backward_inside_the_bound_and_a_reproducible_relation_gradient(dev, c):
    t, ent, rel, s, p, o, (S, P, O) = _case(c, dev)
    d, n, K, slot = c["d"], len(p), c["K"], c["slot"]
    rng = np.random.default_rng(K + d)
    negn, g = rng.integers(0, E, (n, K)), rng.standard_normal((n, K)).astype(np.float32)
    negn[0, K - 1] = negn[0, 0]
    ge0, gr0 = rng.standard_normal((E, d)).astype(np.float32), rng.standard_normal((R, d * d)).astype(np.float32)
    NEG, G = torch.from_numpy(negn).to(dev), torch.from_numpy(g).to(dev)
    pitched = c["layout"] == "pitched"
    ge, gr = _backward(t, S, P, O, slot, NEG, G, ge0, gr0, dev, pitched)
    direction, a = ("sp_", s) if slot == 2 else ("_po", o)
    wa, wm, wx = rr.rows_bwd(direction, ent, rel, a, p, negn, g)
    zero = np.zeros_like
    _within(ge, rr.accum([(np.arange(E), ge0, zero(ge0)), (a, *wa), (negn, wx[0].reshape(-1, d), wx[1].reshape(-1, d))],
                         (E, d)), ("grad_ent", slot))
    _within(gr, rr.accum([(np.arange(R), gr0, zero(gr0)), (p, *wm)], (R, d * d)), ("grad_rel", slot))
    # grad_rel: the same bits on a second run, and with the batch reordered so that every relation keeps its rows' order
    assert torch.equal(_backward(t, S, P, O, slot, NEG, G, ge0, gr0, dev, pitched)[1], gr)
    order = np.argsort(-p, kind="stable")  # relations descending, every relation's rows ascending as before
    T = torch.from_numpy(order).to(dev)
    ge2, gr2 = _backward(t, S[T], P[T], O[T], slot, NEG[T], G[T], ge0, gr0, dev, pitched)
    assert torch.equal(gr2, gr)


def test_the_n_by_1_form_is_the_backward_of_score_spo(dev):
    from kge_amd import engine
    t, ent, rel, s, p, o, (S, P, O) = _case(BASE, dev)
    d, n = BASE["d"], len(p)
    g = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    ge, gr = torch.zeros(E, d, device=dev), torch.zeros(R, d * d, device=dev)
    assert engine.score_neg_bwd_accum_grouped(t, S, P, O, 2, O.view(n, 1), torch.from_numpy(g).to(dev).view(n, 1), None,
                                              ge, gr)
    wa, wm, wx = rr.rows_bwd("sp_", ent, rel, s, p, o[:, None], g[:, None])
    _within(ge, rr.accum([(s, *wa), (o, wx[0][:, 0], wx[1][:, 0])], (E, d)), "spo grad_ent")
    _within(gr, rr.accum([(p, *wm)], (R, d * d)), "spo grad_rel")


def test_model_backward_on_the_grouped_route(dev):
    from kge_amd import model
    d, K = 17, 4
    ent, rel = rr.make_tables(E, R, d, 3)
    m = model.create("rescal", E, R, d, device=dev, grouped=True)
    with torch.no_grad():
        m.get_s_embedder().weight.copy_(torch.from_numpy(ent))
        m.get_p_embedder().weight.copy_(torch.from_numpy(rel))
    p = _relations("random")
    rng = np.random.default_rng(9)
    s, o, negn = rng.integers(0, E, len(p)), rng.integers(0, E, len(p)), rng.integers(0, E, (len(p), K))
    g1, g2 = rng.standard_normal(len(p)).astype(np.float32), rng.standard_normal((len(p), K)).astype(np.float32)
    S, P, O, NEG = (torch.from_numpy(x).to(dev) for x in (s, p, o, negn))
    loss = (m.score_spo(S, P, O) * torch.from_numpy(g1).to(dev)).sum() + \
        (m.score_neg(S, P, O, 0, NEG) * torch.from_numpy(g2).to(dev)).sum()
    loss.backward()
    a1, m1, x1 = rr.rows_bwd("sp_", ent, rel, s, p, o[:, None], g1[:, None])
    a2, m2, x2 = rr.rows_bwd("_po", ent, rel, o, p, negn, g2)
    _within(m.get_s_embedder().weight.grad,
            rr.accum([(s, *a1), (o, x1[0][:, 0], x1[1][:, 0]), (o, *a2), (negn, x2[0].reshape(-1, d), x2[1].reshape(-1, d))],
                     (E, d)), "model grad_ent")
    _within(m.get_p_embedder().weight.grad, rr.accum([(p, *m1), (p, *m2)], (R, d * d)), "model grad_rel")


def test_relational_tucker3_inherits_the_route(dev):
    from kge_amd import model
    d, dr, K = 12, 5, 3
    ent, B, W = tr.make_params(E, R, d, dr, 13)
    m = model.create("relational_tucker3", E, R, d, rel_base_dim=dr, device=dev, grouped=True, project="all")
    with torch.no_grad():
        m.get_s_embedder().weight.copy_(torch.from_numpy(ent))
        m._relation_embedder.base_embedder.weight.copy_(torch.from_numpy(B))
        m._relation_embedder.projection.weight.copy_(torch.from_numpy(W))
    p = _relations("random")
    rng = np.random.default_rng(4)
    s, o, negn = rng.integers(0, E, len(p)), rng.integers(0, E, len(p)), rng.integers(0, E, (len(p), K))
    g = rng.standard_normal((len(p), K)).astype(np.float32)
    S, P, O, NEG = (torch.from_numpy(x).to(dev) for x in (s, p, o, negn))
    (m.score_neg(S, P, O, 2, NEG) * torch.from_numpy(g).to(dev)).sum().backward()
    Ma, eMa = tr.project(B, W)
    ga, gm, gx = tr.rows_bwd("sp_", ent, Ma[p], eMa[p], s, negn, g)
    g_ent = tr.accum([(s, *ga), (negn.reshape(-1), gx[0].reshape(-1, d), gx[1].reshape(-1, d))], (E, d))
    g_b, g_w = tr.project_bwd(B, W, None, *tr.accum([(p, *gm)], (R, d * d)))
    for got, ref, what in ((m.get_s_embedder().weight.grad, g_ent, "ent"),
                           (m._relation_embedder.base_embedder.weight.grad, g_b, "base"),
                           (m._relation_embedder.projection.weight.grad, g_w, "projection")):
        want, e = ref
        err = np.abs(got.double().cpu().numpy().reshape(want.shape) - want)
        assert (err <= tr.bound(e)).all(), (what, float((err / tr.bound(e)).max()))
