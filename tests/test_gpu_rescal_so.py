"""kge_score_so / kge_score_so_bwd_accum for RESCAL tables that opt in (csrc/rescal_so.hip) against the float64
restatement and derived bounds of tests/_rescal_so_ref.py.  Shapes: d = 4, 8 (less than one 16-column group), 20 (a
ragged group), 64 (two K splits, four groups per slice); n = 1, 33 and m = 1, 7, 37 straddle the pair and relation
tiles of all three kernels.  mode "all": rels None, int64 pairs, dense tables (the 16-byte loads).  mode "listed": an
int32 strided rels vector that repeats a relation, int32 pairs, tables with odd pitches (the element loads), out_ld > m
with guard columns."""
import itertools

import numpy as np
import pytest
import torch

import _rescal_ref as RR
import _rescal_so_ref as SO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, R_LISTED = 11, 5
CASES = list(itertools.product((4, 8, 20, 64), (1, 33), (1, 7, 37), ("all", "listed")))


def _case(d, n, m, mode):
    from kge_amd import engine
    listed = mode == "listed"
    R = R_LISTED if listed else m
    ent, rel = RR.make_tables(E, R, d, seed=d + 7 * n + m)
    rng = np.random.default_rng(100 + d + n + m)
    s, o = rng.integers(0, E, n), rng.integers(0, E, n)
    rels = rng.integers(0, R, m) if listed else np.arange(R)
    if listed and m > 1:
        rels[-1] = rels[0]
    if listed:  # odd pitches: no row of either table is 16-byte aligned
        te = torch.zeros(E, d + 3, device=DEV)[:, :d].copy_(torch.from_numpy(ent))
        tr = torch.zeros(R, d * d + 1, device=DEV)[:, :d * d].copy_(torch.from_numpy(rel))
        ix = lambda v: torch.from_numpy(np.repeat(v, 2)).to(DEV, torch.int32)[::2]
    else:
        te, tr = torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV)
        ix = lambda v: torch.from_numpy(v).to(DEV)
    t = engine.Tables("rescal", te, tr)
    return t, ent, rel, s, o, rels, ix(s), ix(o), (ix(rels) if listed else None)


def _ratio(got, ref_err):
    ref, err = ref_err
    return float((np.abs(got.double().cpu().numpy() - ref) / RR.bound(err)).max())


@pytest.mark.parametrize("d,n,m,mode", CASES)
def test_forward(d, n, m, mode):
    from kge_amd import engine
    t, ent, rel, s, o, rels, si, oi, ri = _case(d, n, m, mode)
    pad = 3 if mode == "listed" else 0
    buf = torch.full((n, m + pad), 7.5, device=DEV)
    engine.rescal_score_so(t, si, oi, ri, out=buf[:, :m])
    r = _ratio(buf[:, :m], SO.scores(ent, rel, s, o, rels))
    print("forward d={} n={} m={} {}: err / bound = {:.4f}".format(d, n, m, mode, r))
    assert r < 1.0
    assert bool((buf[:, m:] == 7.5).all())


@pytest.mark.parametrize("d,n,m,mode", CASES)
def test_backward(d, n, m, mode):
    from kge_amd import engine
    t, ent, rel, s, o, rels, si, oi, ri = _case(d, n, m, mode)
    rng = np.random.default_rng(d * n * m)
    g = rng.standard_normal((n, m)).astype(np.float32)
    ge0, gr0 = rng.standard_normal(ent.shape).astype(np.float32), rng.standard_normal(rel.shape).astype(np.float32)
    runs = []
    for _ in range(2):
        ge, gr = torch.from_numpy(ge0).to(DEV), torch.from_numpy(gr0).to(DEV)
        engine.rescal_score_so_bwd(t, si, oi, ri, torch.from_numpy(g).to(DEV), ge, gr)
        runs.append((ge, gr))
    ref_ent, ref_rel = SO.grads(ent, rel, s, o, rels, g, ge0, gr0)
    r = max(_ratio(runs[0][0], ref_ent), _ratio(runs[0][1], ref_rel))
    print("backward d={} n={} m={} {}: err / bound = {:.4f}".format(d, n, m, mode, r))
    assert r < 1.0
    if ri is None:  # one owner per element, a fixed order over the pairs: the same bits on every run
        assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("grad", (False, True))
def test_model_route(grad, monkeypatch):
    """A grouped model's score_so is one engine.rescal_score_so call; scores and parameter gradients match the composed
    path.  Both paths sum the same d^2 (n, m d) products with at most as many roundings as the bound counts, so they
    differ by at most twice the bound."""
    from kge_amd import engine, model
    torch.manual_seed(3)
    mdl = model.create("rescal", 40, 7, 8, device=DEV, grouped=True)
    calls, orig = [], engine.rescal_score_so
    monkeypatch.setattr(engine, "rescal_score_so", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    s, o = torch.arange(9, device=DEV) * 3 % 40, torch.arange(9, device=DEV) * 7 % 40
    g = torch.randn(9, 7, device=DEV)
    res = []
    for fused in (True, False):
        mdl.fused_score_so = fused
        mdl.zero_grad()
        with torch.set_grad_enabled(grad):
            out = mdl.score_so(s, o)
        if grad:
            (out * g).sum().backward()
        res.append((out.detach(), [p.grad.clone() for p in mdl.parameters()] if grad else []))
    assert len(calls) == 1
    ent, rel = (p.detach().cpu().numpy() for p in (mdl.get_s_embedder().weight, mdl.get_p_embedder().weight))
    sn, on, rl = s.cpu().numpy(), o.cpu().numpy(), np.arange(7)
    lim = lambda e: torch.from_numpy(2 * RR.bound(e)).to(DEV)
    assert bool(((res[0][0] - res[1][0]).abs().double() <= lim(SO.scores(ent, rel, sn, on, rl)[1])).all())
    if grad:
        (_, e_ent), (_, e_rel) = SO.grads(ent, rel, sn, on, rl, g.cpu().numpy(), 0 * ent, 0 * rel)
        for a, b, e in zip(res[0][1], res[1][1], (e_ent, e_rel)):
            assert bool(((a - b).abs().double() <= lim(e)).all())
