"""tests/_transh_ref.py (the float64 restatement of TransH and its derived float32 bound) against the reference's own
TransHScorer.score_emb, against the committed fixtures of that scorer's outputs, and against torch autograd (float64) of
the reference's operation sequence; planted defects must exceed the bound on the inputs chosen here."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _transh_ref as th

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
F = torch.nn.functional


# ---- the reference's operation sequence (transh.py:39-78) in torch, any dtype -------------------------------------------
def _proj(e, w):
    wn = F.normalize(w, p=2, dim=-1)
    return e - torch.sum(e * wn, dim=-1, keepdim=True) * wn


def ref_ops(ent, rel, s, p, o, lp, combine, eps=1e-6):
    d = ent.shape[1]
    pe = rel[p]
    r, w = pe[:, :d], pe[:, d:]
    n = pe.shape[0]
    if combine == "spo":
        return -F.pairwise_distance(_proj(ent[s], w) + r, _proj(ent[o], w), p=lp, eps=eps)
    if combine == "sp_":
        T = ent if o is None else ent[o]
        m = T.shape[0]
        q = (_proj(ent[s], w) + r).repeat(m, 1)
        t = _proj(T.repeat_interleave(n, 0), w.repeat(m, 1))
        return -F.pairwise_distance(q, t, p=lp, eps=eps).view(m, n).t()
    T = ent if s is None else ent[s]
    m = T.shape[0]
    q = (_proj(ent[o], w) - r).repeat(m, 1)
    t = _proj(T.repeat_interleave(n, 0), w.repeat(m, 1))
    return -F.pairwise_distance(q, t, p=lp, eps=eps).view(m, n).t()


def _idx(rng, E, R, n):
    return rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)


# ---- scores ---------------------------------------------------------------------------------------------------------
# The reference's scores are a float32 evaluation of the same formulas: its operations are those the bound counts, in
# another summation order (which the bound does not depend on) and with `e - (w^.e) w^` as a product and a difference
# where the kernels write one fma -- one rounding more on a term the bound already carries at |e| + |a w^|.  So the
# reference lies within b of the exact value as the kernels do, and within 2 b of the restatement's float64 value
# once its own deviation and that extra rounding are both granted a full b: the tolerance is 2 b, nothing measured.
@pytest.mark.skipif(not rh.available(), reason="reference tree not present")
@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("d", [32, 33])
def test_restatement_matches_the_reference_scorer(lp, d):
    rh.import_reference()
    from kge.model.transh import TransHScorer
    cfg = rh.make_config("transh", d, {"transh.l_norm": lp})
    scorer = TransHScorer(cfg, None, "transh")
    E, R, n = 23, 4, 7
    ent, rel = th.make_tables(E, R, d, 5)
    rng = np.random.default_rng(6)
    s, p, o = _idx(rng, E, R, n)
    p[0], p[1], s[1], o[1] = 0, 1, 0, 0
    te, tr = torch.from_numpy(ent), torch.from_numpy(rel)
    with torch.no_grad():
        want = {
            "spo": scorer.score_emb(te[s], tr[p], te[o], "spo").view(-1).numpy(),
            "sp": scorer.score_emb(te[s], tr[p], te, "sp_").numpy(),
            "po": scorer.score_emb(te, tr[p], te[o], "_po").numpy(),
        }
    got, b = th.score_spo(lp, ent, rel, s, p, o)
    assert (np.abs(got - want["spo"]) <= 2 * b).all()
    for name, a in (("sp", s), ("po", o)):
        got, b = th.score_pairs(lp, name, ent, rel, a, p)
        assert (np.abs(got - want[name]) <= 2 * b).all(), name
    assert np.isfinite(want["sp"]).all()


@pytest.mark.parametrize("case", ["transh_l1_d32", "transh_l2_d32", "transh_l1_d33", "transh_l2_d33"])
def test_restatement_matches_the_committed_reference_outputs(case):
    z = np.load(os.path.join(GOLDEN, f"{case.replace('transh_', 'transh_scores_')}.npz"))
    lp = float(z["l_norm"])
    ent, rel, s, p, o, sub = (z[k] for k in ("ent", "rel", "s", "p", "o", "sub"))
    assert rel.shape[1] == 2 * ent.shape[1] and not rel[0, ent.shape[1]:].any()
    got, b = th.score_spo(lp, ent, rel, s, p, o)
    assert (np.abs(got - z["spo"]) <= 2 * b).all()
    for key, direction, a, tg in (("sp", "sp", s, None), ("po", "po", o, None), ("sp_sub", "sp", s, sub),
                                  ("po_sub", "po", o, sub)):
        got, b = th.score_pairs(lp, direction, ent, rel, a, p, tg)
        assert got.shape == z[key].shape
        assert (np.abs(got - z[key]) <= 2 * b).all(), key
    m = len(sub)
    assert np.array_equal(z["sp_po_sub"][:, :m], z["sp_sub"]) and np.array_equal(z["sp_po_sub"][:, m:], z["po_sub"])


def test_zero_normal_gives_the_shifted_transe_distance():
    ent, rel = th.make_tables(9, 3, 8, 2)
    s, p, o = np.array([2, 3]), np.array([0, 0]), np.array([4, 5])
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    for lp in (1.0, 2.0):
        got, _ = th.score_spo(lp, ent, rel, s, p, o)
        v = e64[s] + r64[p][:, :8] - e64[o] + th.EPS
        want = -np.abs(v).sum(1) if lp == 1.0 else -np.sqrt((v * v).sum(1))
        assert np.allclose(got, want, rtol=1e-15, atol=0) and np.isfinite(got).all()


# ---- gradients against autograd of the reference's operation sequence ---------------------------------------------------
def _case(d=8, E=11, R=4, n=5, seed=3):
    ent, rel = th.make_tables(E, R, d, seed)
    rng = np.random.default_rng(seed + 1)
    s, p, o = _idx(rng, E, R, n)
    p[0] = 0                      # a zero w row
    s[1], p[1], o[1] = 0, 1, 0    # the zero-distance triple
    return ent, rel, s, p, o, rng


@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("direction", ["sp", "po"])
def test_pairs_gradients_match_autograd(lp, direction):
    ent, rel, s, p, o, rng = _case()
    a = s if direction == "sp" else o
    targets = np.array([0, 3, 3, 7, 1, 0])  # a repeated target, the zero row
    G = rng.standard_normal((len(a), len(targets)))
    te = torch.tensor(ent, dtype=torch.float64, requires_grad=True)
    tr = torch.tensor(rel, dtype=torch.float64, requires_grad=True)
    ta, tp, tt = torch.as_tensor(a), torch.as_tensor(p), torch.as_tensor(targets)
    A, Rr, Tg = te[ta], tr[tp], te[tt]
    for x in (A, Rr, Tg):
        x.retain_grad()
    d = ent.shape[1]
    w = Rr[:, d:]
    m, n = len(targets), len(a)
    sign = 1.0 if direction == "sp" else -1.0
    q = (_proj(A, w) + sign * Rr[:, :d]).repeat(m, 1)
    t = _proj(Tg.repeat_interleave(n, 0), w.repeat(m, 1))
    sc = -F.pairwise_distance(q, t, p=lp, eps=th.EPS).view(m, n).t()
    (sc * torch.as_tensor(G)).sum().backward()
    (g_a, g_p, g_t), _, safe = th.pairs_bwd(lp, direction, ent, rel, a, p, targets, G)
    assert safe
    big = np.linalg.norm(rel[p][:, d:].astype(np.float64), axis=1) >= th.NORM_EPS
    assert np.allclose(g_a, A.grad.numpy(), rtol=1e-9, atol=1e-11)
    assert np.allclose(g_t, Tg.grad.numpy(), rtol=1e-9, atol=1e-11)
    assert np.allclose(g_p[:, :d], Rr.grad.numpy()[:, :d], rtol=1e-9, atol=1e-11)
    assert np.allclose(g_p[big, d:], Rr.grad.numpy()[big, d:], rtol=1e-9, atol=1e-11)
    # a zero w row: the normalisation divides by its eps, the gradient is g_w^ / 1e-12 (torch: the same clamp)
    assert np.allclose(g_p[~big, d:], Rr.grad.numpy()[~big, d:], rtol=1e-9, atol=1e-3)


@pytest.mark.parametrize("lp", [1.0, 2.0])
@pytest.mark.parametrize("slot", [0, 2])
def test_triple_gradients_match_autograd(lp, slot):
    ent, rel, s, p, o, rng = _case()
    K = 3
    neg = rng.integers(0, ent.shape[0], (len(s), K))
    neg[1, 0] = 0  # the zero-distance triple among the negatives
    G = rng.standard_normal((len(s), K))
    te = torch.tensor(ent, dtype=torch.float64, requires_grad=True)
    tr = torch.tensor(rel, dtype=torch.float64, requires_grad=True)
    idx = [np.repeat(x, K) for x in (s, p, o)]
    idx[slot] = neg.reshape(-1)
    sc = ref_ops(te, tr, torch.as_tensor(idx[0]), torch.as_tensor(idx[1]), torch.as_tensor(idx[2]), lp, "spo", th.EPS)
    (sc * torch.as_tensor(G.reshape(-1))).sum().backward()
    (ge, gr), _, safe = th.neg_bwd_accum(lp, ent, rel, s, p, o, slot, neg, G)
    assert safe
    d = ent.shape[1]
    big = np.linalg.norm(rel[:, d:].astype(np.float64), axis=1) >= th.NORM_EPS
    assert np.allclose(ge, te.grad.numpy(), rtol=1e-9, atol=1e-11)
    assert np.allclose(gr[:, :d], tr.grad.numpy()[:, :d], rtol=1e-9, atol=1e-11)
    assert np.allclose(gr[big, d:], tr.grad.numpy()[big, d:], rtol=1e-9, atol=1e-11)
    assert np.allclose(gr[~big, d:], tr.grad.numpy()[~big, d:], rtol=1e-9, atol=1e-3)
    # spo_bwd = the K = 1 case, per row
    (g_s, g_p, g_o), _, _ = th.spo_bwd(lp, ent, rel, s, p, o, G[:, 0])
    (ge1, gr1), _, _ = th.neg_bwd_accum(lp, ent, rel, s, p, o, 2, o[:, None], G[:, :1])
    ge2 = np.zeros_like(ge1)
    np.add.at(ge2, s, g_s)
    np.add.at(ge2, o, g_o)
    assert np.allclose(ge1, ge2, rtol=1e-12, atol=1e-13)


# ---- planted defects exceed the bound ---------------------------------------------------------------------------------
def _defect_inputs():
    ent, rel = th.make_tables(13, 4, 16, 7, zero_pair=False)
    rng = np.random.default_rng(8)
    n = 6
    s, p, o = _idx(rng, 13, 4, n)
    p[:] = rng.integers(1, 4, n)  # relations with a hyperplane
    G = rng.standard_normal((n, 13)) + 2.0
    return ent, rel, s, p, o, G


def test_defect_eps_on_the_wrong_side_of_po_exceeds_the_bound():
    ent, rel, s, p, o, _ = _defect_inputs()
    # coordinates of the size of EPS make its placement visible: small tables
    ent, rel = (ent * np.float32(2e-5)).astype(np.float32), rel.copy()
    rel[:, :16] *= np.float32(2e-5)
    for lp in (1.0, 2.0):
        good, b = th.score_pairs(lp, "po", ent, rel, o, p)
        bad, _ = th.score_pairs(lp, "po", ent, rel, o, p, defect={"po_eps_wrong_side": True})
        assert (np.abs(good - bad) > b).mean() > 0.9


def test_defect_projection_dropped_from_the_target_gradient_exceeds_the_bound():
    ent, rel, s, p, o, G = _defect_inputs()
    for lp in (1.0, 2.0):
        (_, _, good), (_, _, b), safe = th.pairs_bwd(lp, "sp", ent, rel, s, p, None, G)
        (_, _, bad), _, _ = th.pairs_bwd(lp, "sp", ent, rel, s, p, None, G, defect={"no_P_in_g_x": True})
        assert safe and (np.abs(good - bad) > b).mean() > 0.9


def test_defect_normalisation_jacobian_dropped_exceeds_the_bound():
    ent, rel, s, p, o, G = _defect_inputs()
    d = ent.shape[1]
    for lp in (1.0, 2.0):
        (_, good, _), (_, b, _), _ = th.pairs_bwd(lp, "sp", ent, rel, s, p, None, G)
        (_, bad, _), _, _ = th.pairs_bwd(lp, "sp", ent, rel, s, p, None, G, defect={"no_normalize_jacobian": True})
        assert (np.abs(good - bad)[:, d:] > b[:, d:]).mean() > 0.9
        assert np.array_equal(good[:, :d], bad[:, :d])
