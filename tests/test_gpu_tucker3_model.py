"""model.RelationalTucker3 on the GPU: every score_* and the gradients of all three parameters against the float64
restatement (tests/_tucker3_ref.py) on both routes, the routes against each other and against model.Rescal on the
projected table, and the cache of the projected table."""
import numpy as np
import pytest
import torch

import _tucker3_ref as tr

pytestmark = pytest.mark.gpu

E, D, DR, K = 37, 8, 5, 6
CASES = [(5, 11), (70, 64)]  # (R, n): R <= n ("all" under "auto") and R > n ("batch")
KINDS = ("sp", "po", "spo", "neg0", "neg2")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


_DATA = {}


def _data(R, n):
    if (R, n) not in _DATA:
        ent, B, W = tr.make_params(E, R, D, DR, 11 * R + n)
        rng = np.random.default_rng(R + n)
        s, p, o = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
        p[0], p[2], s[2] = 1, p[1], s[1]  # the zero base row; a repeated relation with a repeated entity
        neg = rng.integers(0, E, (n, K))
        g = {"sp": rng.standard_normal((n, E)), "po": rng.standard_normal((n, E)), "spo": rng.standard_normal(n),
             "neg0": rng.standard_normal((n, K)), "neg2": rng.standard_normal((n, K))}
        g = {k: v.astype(np.float32) for k, v in g.items()}
        _DATA[(R, n)] = (ent, B, W, s, p, o, neg, g)
    return _DATA[(R, n)]


def _model(R, n, dev, **kw):
    from kge_amd import model
    ent, B, W = _data(R, n)[:3]
    m = model.create("relational_tucker3", E, R, D, rel_base_dim=DR, device=dev, **kw)
    with torch.no_grad():
        m._entity_embedder.weight.copy_(torch.from_numpy(ent))
        m._relation_embedder.base_embedder.weight.copy_(torch.from_numpy(B))
        m._relation_embedder.projection.weight.copy_(torch.from_numpy(W))
    return m


def _params(m):
    return (m._entity_embedder.weight, m._relation_embedder.base_embedder.weight, m._relation_embedder.projection.weight)


def _score(m, kind, idx, route):
    s, p, o, neg = idx
    if kind == "sp":
        return m.score_sp(s, p, project=route)
    if kind == "po":
        return m.score_po(p, o, project=route)
    if kind == "spo":
        return m.score_spo(s, p, o, project=route)
    return m.score_neg(s, p, o, 0 if kind == "neg0" else 2, neg, project=route)


_REFS = {}


def _ref(R, n, kinds, route):
    """(scores per kind, (g_ent, e), (g_B, e), (g_W, e)) of sum_kind sum(gout_kind * score_kind), computed once"""
    key = (R, n, kinds, route)
    if key in _REFS:
        return _REFS[key]
    ent, B, W, s, p, o, neg, g = _data(R, n)
    if route == "all":
        Ma, eMa = tr.project(B, W)
        M, eM = Ma[p], eMa[p]
    else:
        M, eM = tr.project(B, W, p)
    scores, eparts, mparts = {}, [], []
    rel_ids = p if route == "all" else np.arange(n)
    for kind in kinds:
        if kind in ("sp", "po"):
            direction, a = ("sp_", s) if kind == "sp" else ("_po", o)
            scores[kind] = tr.score_pairs(direction, ent, M, eM, a)
            ga, gm, gt = tr.pairs_bwd(direction, ent, M, eM, a, None, g[kind])
            eparts += [(np.arange(E), *gt), (a, *ga)]
        else:
            direction, a = ("_po", o) if kind == "neg0" else ("sp_", s)
            x = o[:, None] if kind == "spo" else neg
            scores[kind] = tr.score_rows(direction, ent, M, eM, a, o if kind == "spo" else neg)
            ga, gm, gx = tr.rows_bwd(direction, ent, M, eM, a, x, g[kind].reshape(n, -1))
            eparts += [(a, *ga), (x.reshape(-1), gx[0].reshape(-1, D), gx[1].reshape(-1, D))]
        mparts.append((rel_ids, *gm))
    g_ent = tr.accum(eparts, (E, D))
    GM, eGM = tr.accum(mparts, (R if route == "all" else n, D * D))
    if route == "all":
        g_b, g_w = tr.project_bwd(B, W, None, GM, eGM)
    else:
        rows, g_w = tr.project_bwd(B, W, p, GM, eGM)
        g_b = tr.base_grad(R, p, *rows)
    _REFS[key] = (scores, g_ent, g_b, g_w)
    return _REFS[key]


def _within(got, ref, what):
    want, e = ref
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    err, tol = np.abs(got - want), tr.bound(e)
    bad = err > tol
    assert not bad.any(), "{}: {} of {} outside the bound (worst {:.3e} at a bound of {:.3e})".format(
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(tol[bad][err[bad].argmax()]))


def _idx(R, n, dev):
    return tuple(torch.from_numpy(x).to(dev) for x in _data(R, n)[3:7])


@pytest.mark.parametrize("R,n", CASES)
@pytest.mark.parametrize("route", ["all", "batch"])
@pytest.mark.parametrize("kind", KINDS)
def test_scores_and_gradients(dev, R, n, route, kind):
    m = _model(R, n, dev)
    idx = _idx(R, n, dev)
    scores, g_ent, g_b, g_w = _ref(R, n, (kind,), route)
    out = _score(m, kind, idx, route)
    _within(out, scores[kind], "{} scores".format(kind))
    (out * torch.from_numpy(_data(R, n)[7][kind]).to(dev)).sum().backward()
    for prm, ref, name in zip(_params(m), (g_ent, g_b, g_w), ("entity", "base", "projection")):
        _within(prm.grad, ref, "{} ({}): {} gradient".format(kind, route, name))


@pytest.mark.parametrize("R,n", CASES)
@pytest.mark.parametrize("route", ["all", "batch"])
def test_neg_blocks_and_sp_po(dev, R, n, route):
    m = _model(R, n, dev)
    s, p, o, neg = idx = _idx(R, n, dev)
    g = _data(R, n)[7]
    pos, ns, no = m.score_neg_blocks(s, p, o, neg, neg, project=route)
    with torch.no_grad():
        assert torch.equal(pos, _score(m, "spo", idx, route)) and torch.equal(ns, _score(m, "neg0", idx, route)) \
            and torch.equal(no, _score(m, "neg2", idx, route)), "score_neg_blocks = the single calls"
        both = m.score_sp_po(s, p, o, project=route)
        assert torch.equal(both[:, :E], _score(m, "sp", idx, route)) and \
            torch.equal(both[:, E:], _score(m, "po", idx, route)), "score_sp_po = [score_sp | score_po]"
    both_g = m.score_sp_po(s, p, o, project=route)  # with a gradient: the composed form
    assert both_g.requires_grad and torch.equal(both_g.detach(), both)
    gt = {k: torch.from_numpy(v).to(dev) for k, v in g.items()}
    ((pos * gt["spo"]).sum() + (ns * gt["neg0"]).sum() + (no * gt["neg2"]).sum()).backward()
    _, g_ent, g_b, g_w = _ref(R, n, ("spo", "neg0", "neg2"), route)
    for prm, ref, name in zip(_params(m), (g_ent, g_b, g_w), ("entity", "base", "projection")):
        _within(prm.grad, ref, "score_neg_blocks ({}): {} gradient".format(route, name))


@pytest.mark.parametrize("R,n", CASES)
def test_routes_agree_and_equal_rescal(dev, R, n):
    from kge_amd import engine, model
    m = _model(R, n, dev)
    s, p, o, neg = idx = _idx(R, n, dev)
    B, W = _params(m)[1:]
    ident = torch.arange(n, device=dev)
    with torch.no_grad():
        table, rows = engine.tucker3_project(B, W), engine.tucker3_project(B, W, p)
        assert torch.equal(table[p], rows)
        rs = {"all": (model.create("rescal", E, R, D, device=dev), table, p),
              "batch": (model.create("rescal", E, n, D, device=dev), rows, ident)}
        for route, (r, rel, p2) in rs.items():
            r._entity_embedder.weight.copy_(m._entity_embedder.weight)
            r._relation_embedder.weight.copy_(rel)
            ridx = (s, p2, o, neg)
            for kind in KINDS:
                assert torch.equal(_score(m, kind, idx, route), _score_rescal(r, kind, ridx)), \
                    "{} ({}): bit-equal to model.Rescal on the projected table".format(kind, route)
    for kind in KINDS:
        a, b = _score(m, kind, idx, "all"), _score(m, kind, idx, "batch")
        ea, eb = _ref(R, n, (kind,), "all")[0][kind][1], _ref(R, n, (kind,), "batch")[0][kind][1]
        diff = (a.double() - b.double()).abs().detach().cpu().numpy().reshape(ea.shape)
        assert (diff <= tr.bound(ea) + tr.bound(eb)).all(), "{}: the routes agree within the sum of their bounds".format(kind)
    assert m.route(n) == ("all" if R <= n else "batch")
    with torch.no_grad():
        assert m.route(n) == "all"


def _score_rescal(r, kind, idx):
    s, p, o, neg = idx
    if kind == "sp":
        return r.score_sp(s, p)
    if kind == "po":
        return r.score_po(p, o)
    if kind == "spo":
        return r.score_spo(s, p, o)
    return r.score_neg(s, p, o, 0 if kind == "neg0" else 2, neg)


def test_projected_table_cache(dev):
    R, n = 70, 64
    m = _model(R, n, dev)
    s, p, o, _ = _idx(R, n, dev)
    with torch.no_grad():
        a = m.score_sp(s, p).clone()
        assert m.projections == 1
        b = m.score_sp_po(s, p, o)
        c = m.score_po(p, o)
        assert m.projections == 1, "an evaluation projects once"
        assert torch.equal(b[:, :E], a) and torch.equal(b[:, E:], c)
    live = m.score_sp(s, p, project="all")  # a gradient is recorded: projected anew, nothing cached
    assert m.projections == 1 and torch.equal(live.detach(), a), "bit-equal scores with and without the cache"
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    live.sum().backward()
    opt.step()
    with torch.no_grad():
        d = m.score_sp(s, p)
        assert m.projections == 2, "rebuilt after optimizer.step()"
        assert not torch.equal(d, a)
        fresh = m.score_sp(s, p, project="batch")
        assert torch.equal(d, fresh), "the rebuilt table is the parameters' projection"
        m.score_sp(s, p)
        assert m.projections == 2


def test_limits(dev):
    from kge_amd import model
    for opt in ("fused_dist_loss", "fused_f32_loss"):
        with pytest.raises(ValueError, match=opt):
            model.create("relational_tucker3", E, 5, D, rel_base_dim=DR, device=dev, **{opt: True})
    with pytest.raises(ValueError, match="dim"):
        model.create("relational_tucker3", E, 5, 257, rel_base_dim=DR, device="meta")
    m = _model(5, 11, dev)
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(E, D, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)))
    s, p, o, neg = _idx(5, 11, dev)
    with pytest.raises(ValueError, match="score_neg_shared"):
        m.score_neg_shared(s, p, o, 2, neg[0])
    r = model.create("rescal", E, 5, D, device=dev)  # predict_o / predict_s: the composed path, as model.Rescal
    with torch.no_grad():
        r._entity_embedder.weight.copy_(m._entity_embedder.weight)
        r._relation_embedder.weight.copy_(m.projected_table())
    for got, want in zip(m.predict_o(s, p, 3) + m.predict_s(p, o, 3), r.predict_o(s, p, 3) + r.predict_s(p, o, 3)):
        assert torch.equal(got, want)


def test_batch_route_skips_the_wide_scatter(dev, monkeypatch):
    """"batch": the [n, d^2] relation gradient of score_sp / score_po goes to the projection backward as it is -- no
    d^2-wide index_add_ (the "all" route has one)"""
    from kge_amd import model
    R, n = 70, 64
    m = _model(R, n, dev)
    s, p, o, _ = _idx(R, n, dev)
    widths = []
    real = model._scatter_rows

    def spy(table, idx, rows):
        widths.append(rows.shape[1])
        return real(table, idx, rows)

    monkeypatch.setattr(model, "_scatter_rows", spy)
    for route, wide in (("batch", 0), ("all", 2)):
        del widths[:]
        (m.score_sp(s, p, project=route).sum() + m.score_po(p, o, project=route).sum()).backward()
        assert widths.count(D * D) == wide, (route, widths)
        assert DR in widths or route == "all", "the base rows' gradient is scattered (d_r wide)"
