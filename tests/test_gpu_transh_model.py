"""kge_amd.model.TransH on the GPU: the five scoring methods and their autograd against tests/_transh_ref.py, two training
steps, link prediction and the stand-alone evaluator on the composed path, the refused options."""
import numpy as np
import pytest
import torch

import _transh_ref as th

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(E, R, d, lp, seed=0):
    from kge_amd import model
    torch.manual_seed(seed)
    m = model.create("transh", E, R, d, l_norm=lp, device=DEV)
    ent, rel = th.make_tables(E, R, d, seed + 3, zero_pair=False)
    with torch.no_grad():
        m.get_s_embedder().weight.copy_(torch.from_numpy(ent))
        m.get_p_embedder().weight.copy_(torch.from_numpy(rel))
    return m, ent, rel


def _within(got, want, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("lp", [1.0, 2.0])
def test_scores_and_autograd_against_the_restatement(lp):
    E, R, d, n, K = 40, 5, 33, 9, 4
    m, ent, rel = _model(E, R, d, lp)
    assert tuple(m.get_p_embedder().weight.shape) == (R, 2 * d)
    rng = np.random.default_rng(2)
    s, p, o = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    neg = rng.integers(0, E, (n, K))
    S, P, O, NEG = (torch.from_numpy(x).to(DEV) for x in (s, p, o, neg))
    We, Wr = m.get_s_embedder().weight, m.get_p_embedder().weight
    U = th.U

    def grads(out, G):
        We.grad = Wr.grad = None
        (out * torch.from_numpy(G).to(DEV)).sum().backward()
        return We.grad.clone(), Wr.grad.clone()

    # score_spo, score_neg (both slots): scores and table gradients
    for slot, ng, call in ((2, o[:, None], lambda: m.score_spo(S, P, O).view(n, 1)),
                           (0, neg, lambda: m.score_neg(S, P, O, 0, NEG)), (2, neg, lambda: m.score_neg(S, P, O, 2, NEG))):
        out = call()
        want, b = th.score_neg(lp, ent, rel, s, p, o, slot, ng)
        _within(out, want, b, "score")
        G = rng.standard_normal(want.shape).astype(np.float32)
        ge, gr = grads(out, G)
        (w_e, w_r), (b_e, b_r), safe = th.neg_bwd_accum(lp, ent, rel, s, p, o, slot, ng, G)
        assert safe
        _within(ge, w_e, b_e + 2 * U * (np.abs(w_e) + b_e), "grad ent")
        _within(gr, w_r, b_r + 2 * U * (np.abs(w_r) + b_r), "grad rel")
    # score_sp / score_po / score_sp_po: scores, and gradients scattered into the tables by the autograd node
    sub = torch.tensor([3, 0, 3, 17], device=DEV)
    for direction, a, call in (("sp", s, lambda t: m.score_sp(S, P, t)), ("po", o, lambda t: m.score_po(P, O, t))):
        for tg in (None, sub):
            out = call(tg)
            tgn = None if tg is None else tg.cpu().numpy()
            want, b = th.score_pairs(lp, direction, ent, rel, a, p, tgn)
            _within(out, want, b, direction)
            G = rng.standard_normal(want.shape).astype(np.float32)
            ge, gr = grads(out, G)
            (w_a, w_p, w_t), (b_a, b_p, b_t), safe = th.pairs_bwd(lp, direction, ent, rel, a, p, tgn, G)
            assert safe
            we, be, wr, br = np.zeros(ent.shape), np.zeros(ent.shape), np.zeros(rel.shape), np.zeros(rel.shape)
            mag = np.zeros(ent.shape)
            rows = np.arange(E) if tgn is None else tgn
            for idx, w, bb in ((rows, w_t, b_t), (a, w_a, b_a)):
                np.add.at(we, idx, w)
                np.add.at(be, idx, bb)
                np.add.at(mag, idx, np.abs(w))
            np.add.at(wr, p, w_p)
            np.add.at(br, p, b_p)
            magr = np.zeros(rel.shape)
            np.add.at(magr, p, np.abs(w_p))
            _within(ge, we, be + (n + 4) * U * mag, "pairs grad ent")   # index_add_: at most n + 4 terms per row
            _within(gr, wr, br + n * U * magr, "pairs grad rel")
    with torch.no_grad():
        both = m.score_sp_po(S, P, O, sub)
        assert torch.equal(both, torch.cat((m.score_sp(S, P, sub), m.score_po(P, O, sub)), 1))


@pytest.mark.parametrize("kind", ["negative_sampling", "1vsAll"])
def test_a_training_step_lowers_the_loss(kind):
    from kge_amd import optim
    E, R, d = 40, 4, 16
    m, _, _ = _model(E, R, d, 2.0, seed=1)
    rng = np.random.default_rng(5)
    tri = torch.from_numpy(np.stack([rng.integers(0, E, 64), rng.integers(0, R, 64), rng.integers(0, E, 64)], 1)).to(DEV)
    s, p, o = tri[:, 0], tri[:, 1], tri[:, 2]
    neg = torch.from_numpy(rng.integers(0, E, (64, 8))).to(DEV)
    opt = optim.Adagrad(m.parameters(), lr=0.05)

    def loss():
        if kind == "1vsAll":
            return torch.nn.functional.cross_entropy(m.score_sp(s, p), o) + \
                torch.nn.functional.cross_entropy(m.score_po(p, o), s)
        pos, ns, no = m.score_neg_blocks(s, p, o, neg, neg)
        x = torch.cat((pos.view(-1, 1), ns, no), 1)
        return torch.nn.functional.cross_entropy(x, torch.zeros(64, dtype=torch.long, device=DEV))

    first = loss()
    first.backward()
    opt.step()
    opt.zero_grad()
    with torch.no_grad():
        second = loss()
    assert torch.isfinite(first) and torch.isfinite(second) and float(second) < float(first)


def test_predict_and_the_evaluator_take_the_composed_path():
    from kge_amd import engine, model
    from kge_amd.eval import EntityRankingEvaluator, get_ranks
    from kge_amd.synthetic import make_splits
    E, R, d = 40, 4, 16
    m, _, _ = _model(E, R, d, 1.0, seed=2)
    m.eval()
    splits = make_splits(E, R, 120, 30, 30, seed=3)
    s, p, o = (torch.from_numpy(splits["valid"][:, k]).to(DEV) for k in range(3))
    with torch.no_grad():
        val, idx = m.predict_o(s, p, 5)
        v2, i2 = model.topk_composed(m.score_sp(s, p), 5)
        assert torch.equal(val, v2) and torch.equal(idx, i2)
        val, idx = m.predict_s(p, o, 3)
        v2, i2 = model.topk_composed(m.score_po(p, o), 3)
        assert torch.equal(val, v2) and torch.equal(idx, i2)
        ev = EntityRankingEvaluator(m, splits, E, R, eval_split="valid", batch_size=16)
        metrics, ranks = ev.run(return_ranks=True)
        assert all(np.isfinite(v) for v in metrics.values())
        n = s.numel()
        for side, sc, true_col in (("o", m.score_sp(s, p).contiguous(), o), ("s", m.score_po(p, o).contiguous(), s)):
            rank = torch.zeros(1, n, dtype=torch.int64, device=DEV)
            ties = torch.zeros(1, n, dtype=torch.int64, device=DEV)
            true = sc.gather(1, true_col.view(-1, 1)).view(-1).contiguous()
            engine.rank_counts_multi(sc, true, [], 0, true_col, ev.tie_atol, ev.tie_rtol, rank, ties)
            assert np.array_equal(np.asarray(ranks[side + "_raw"]).reshape(-1), get_ranks(rank, ties)[0].cpu().numpy())


def test_refused_options_name_themselves():
    from kge_amd import engine, model
    with pytest.raises(ValueError, match="fused_dist_loss"):
        model.create("transh", 10, 2, 8, device=DEV, fused_dist_loss=True)
    m, _, _ = _model(10, 2, 8, 1.0)
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(10, 8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)))
    s = torch.zeros(2, dtype=torch.long, device=DEV)
    neg = torch.zeros(2, 3, dtype=torch.long, device=DEV)
    out = m.score_neg(s, s, s, 2, neg)
    old = engine.NEG_BWD_SORTED
    engine.NEG_BWD_SORTED = True
    try:
        with pytest.raises(ValueError, match="NEG_BWD_SORTED"):
            out.sum().backward()
    finally:
        engine.NEG_BWD_SORTED = old
