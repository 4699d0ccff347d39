"""kge_amd.model.KgeModel with fused_dropout=True on the GPU: score_spo and the negative-sampling scores in training mode
equal the reference's op sequence (oracle/torch_port.py) on rows masked as engine.embed_dropout masks them, gradients by
torch autograd through those rows, at the tolerances tests/test_gpu_model_eval.py uses for the undropped comparison
(scores: atol 1e-5, rtol 1e-4; gradients: 2e-4 * max(1, |g|_max)).  Eval mode and p = 0 are bit-equal to the existing
route; two forward calls draw different masks; a node's backward uses its forward's mask."""
import pytest
import torch

import torch_port as tp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E, R, D_, N, K = 40, 5, 36, 19, 7
CASES = [("complex", 1.0, 0.3, 0.2), ("distmult", 1.0, 0.0, 0.4), ("transe", 1.0, 0.3, 0.2), ("transe", 2.0, 0.25, 0.0),
         ("rotate", 1.0, 0.0, 0.3)]  # (RotatE: no entity mask -- a coordinate with s and o both dropped has |q - o| = 0,
#                                       where torch's own norm backward is NaN: nothing to compare with)


def _model(name, l_norm, p_ent, p_rel, fused_dropout=True):
    from kge_amd import model
    torch.manual_seed(5)
    m = model.create(name, E, R, D_, l_norm=l_norm, fused_dropout=fused_dropout, entity_args={"dropout": p_ent},
                     relation_args={"dropout": p_rel}).to(DEV)
    m.dropout_seed = 0x5EED_0000_0000_0001
    return m


def _factors(m, table, idx, role, dropout):
    """the mask factors of engine.embed_dropout: the masked rows of a table of ones"""
    from kge_amd import engine as eng
    ent, rel = m.get_s_embedder().weight, m.get_p_embedder().weight
    ones = eng.Tables(m.get_scorer().name, torch.ones_like(ent), torch.ones_like(rel), l_norm=m.get_scorer()._norm)
    return eng.embed_dropout(ones, table, idx, role, 0, dropout)


def _indices():
    g = torch.Generator().manual_seed(4)
    s = torch.randint(10, (N,), generator=g)
    o = (s + 1 + torch.randint(8, (N,), generator=g)) % 10  # never s: RotatE with a dropped phase scores s against o
    p = torch.randint(R, (N,), generator=g)
    neg = torch.randint(10, E, (N, K), generator=g)  # disjoint from the positives' entities
    neg[:, 1] = neg[:, 0]
    return s.to(DEV), p.to(DEV), o.to(DEV), neg.to(DEV)


def _check_grads(m, ent, rel):
    for got, want, nm in ((m.get_s_embedder().weight.grad, ent.grad, "entity"), (m.get_p_embedder().weight.grad, rel.grad, "relation")):
        scale = max(1.0, float(want.abs().max()))
        err = float((got - want).abs().max())
        assert err <= 2e-4 * scale, (nm, err, scale)


@pytest.mark.parametrize("name,l_norm,p_ent,p_rel", CASES)
def test_training_mode_scores_and_gradients(name, l_norm, p_ent, p_rel):
    from kge_amd import engine as eng
    m = _model(name, l_norm, p_ent, p_rel).train()
    s, p, o, neg = _indices()
    assert m._dropout_triple() == (p_ent, p_rel)
    ent0, rel0 = m.get_s_embedder().weight.detach().clone(), m.get_p_embedder().weight.detach().clone()
    # ---- score_spo
    call0 = m._dropout_clock.call
    w = torch.randn(N, device=DEV)
    got = m.score_spo(s, p, o)
    assert m._dropout_clock.call == call0 + 1
    D = eng.Dropout(p_ent, p_rel, m.dropout_seed, call0 + 1)
    ent, rel = ent0.clone().requires_grad_(), rel0.clone().requires_grad_()
    ref = tp.score_emb(name, ent[s] * _factors(m, "ent", s, 0, D), rel[p] * _factors(m, "rel", p, 1, D),
                       ent[o] * _factors(m, "ent", o, 2, D), "spo", l_norm).view(-1)
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-4)
    m.zero_grad()
    (got * w).sum().backward()
    (ref * w).sum().backward()
    _check_grads(m, ent, rel)
    again = m.score_spo(s, p, o)
    assert not torch.equal(got, again)  # the next call, another mask
    # ---- the negative-sampling scores, both slots
    for slot in (0, 2):
        call0 = m._dropout_clock.call
        w = torch.randn(N, K, device=DEV)
        got = m.score_neg(s, p, o, slot, neg)
        D = eng.Dropout(p_ent, p_rel, m.dropout_seed, call0 + 1)
        ent, rel = ent0.clone().requires_grad_(), rel0.clone().requires_grad_()
        rep = lambda x: x.repeat_interleave(K, dim=0)
        fixed_ids, role_fixed = (o, 2) if slot == 0 else (s, 0)
        fixed = rep(ent[fixed_ids] * _factors(m, "ent", fixed_ids, role_fixed, D))  # masked once per positive
        prow = rep(rel[p] * _factors(m, "rel", p, 1, D))
        flat = neg.reshape(-1)
        var = ent[flat] * _factors(m, "ent", flat, slot, D)  # every occurrence on its own
        rows = (var, prow, fixed) if slot == 0 else (fixed, prow, var)
        ref = tp.score_emb(name, *rows, "spo", l_norm).view(N, K)
        assert torch.allclose(got, ref, atol=1e-5, rtol=1e-4), slot
        m.zero_grad()
        (got * w).sum().backward()
        (ref * w).sum().backward()
        _check_grads(m, ent, rel)
        if p_ent > 0:
            assert not torch.equal(got[:, 0], got[:, 1])  # the same entity twice in a row: two masks


@pytest.mark.parametrize("name,l_norm,p_ent,p_rel", CASES[:3])
def test_eval_mode_and_zero_probability_are_the_existing_route(name, l_norm, p_ent, p_rel):
    from kge_amd import engine as eng
    s, p, o, neg = _indices()
    m = _model(name, l_norm, p_ent, p_rel).eval()
    plain = _model(name, l_norm, p_ent, p_rel, fused_dropout=False).eval()
    calls = m._dropout_clock.call
    assert m._dropout_triple() is None
    assert torch.equal(m.score_spo(s, p, o), eng.score_spo(m.tables(), s, p, o))
    assert torch.equal(m.score_spo(s, p, o), plain.score_spo(s, p, o))
    assert torch.equal(m.score_neg(s, p, o, 2, neg), eng.score_neg(m.tables(), s, p, o, 2, neg))
    z = _model(name, l_norm, 0.0, 0.0).train()
    assert z._dropout_triple() is None
    assert torch.equal(z.score_spo(s, p, o), eng.score_spo(z.tables(), s, p, o))
    assert torch.equal(z.score_neg(s, p, o, 0, neg), eng.score_neg(z.tables(), s, p, o, 0, neg))
    assert m._dropout_clock.call == calls and z._dropout_clock.call == 0
    # without the option a model in training mode takes the composed path: torch's own masks, no fused call
    plain.train()
    assert plain._dropout_triple() is None
    plain.score_spo(s, p, o)
    assert plain._dropout_clock.call == 0
