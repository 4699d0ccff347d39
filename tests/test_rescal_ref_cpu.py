"""tests/_rescal_ref.py checked without a GPU: against the reference's RescalScorer.score_emb, against float64 autograd of
that operation sequence, against committed outputs of the reference model (tests/golden/rescal_scores_*.npz), and by
planted defects that must exceed the bound."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

import _rescal_ref as rr
from conftest import ROOT

E, R, D, N = 11, 4, 6, 7


def _case(seed=3, d=D):
    ent, rel = rr.make_tables(E, R, d, seed)
    rng = np.random.default_rng(seed)
    s, p, o = rng.integers(0, E, N), rng.integers(0, R, N), rng.integers(0, E, N)
    p[:3] = [1, 2, 0]
    return ent, rel, s, p, o


def _torch_scores(scorer, ent, rel, s, p, o, combine):
    e, r = torch.from_numpy(ent).double(), torch.from_numpy(rel).double()
    if combine == "spo":
        return scorer.score_emb(e[s], r[p], e[o], "spo").view(-1)
    if combine == "sp_":
        return scorer.score_emb(e[s], r[p], e, "sp_")
    return scorer.score_emb(e, r[p], e[o], "_po")


def _scorer(which):
    if which == "front end":
        from kge_amd import model
        return model.RescalScorer(1.0)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness as rh
    if not rh.available():
        pytest.skip("reference not on this machine")
    rh.import_reference()
    from kge.model.rescal import RescalScorer
    ref = RescalScorer.__new__(RescalScorer)
    torch.nn.Module.__init__(ref)
    return ref


@pytest.mark.parametrize("which", ["front end", "reference"])
def test_restatement_equals_the_scorers_in_float64(which):
    ent, rel, s, p, o = _case()
    for sc in (_scorer(which),):
        for combine, got in (("spo", rr.score_spo(ent, rel, s, p, o)), ("sp_", rr.score_pairs("sp_", ent, rel, s, p)),
                             ("_po", rr.score_pairs("_po", ent, rel, o, p))):
            want = _torch_scores(sc, ent, rel, s, p, o, combine).numpy()
            assert np.allclose(got[0], want, rtol=1e-12, atol=1e-12), (type(sc), combine)
            assert (got[1] > 0).any() and (got[1] < 1e-3).all()
    # the zero matrix scores exactly zero with a zero bound; the identity is the plain dot product
    sp = rr.score_pairs("sp_", ent, rel, s, p)
    assert not sp[0][0].any() and not sp[1][0].any()
    assert np.allclose(sp[0][1], ent.astype(np.float64)[s[1]] @ ent.astype(np.float64).T)


def test_gradients_equal_float64_autograd():
    ent, rel, s, p, o = _case()
    from kge_amd import model
    sc = model.RescalScorer(1.0)
    rng = np.random.default_rng(0)
    for direction, a in (("sp_", s), ("_po", o)):
        e = torch.from_numpy(ent).double().requires_grad_()
        r = torch.from_numpy(rel).double().requires_grad_()
        ea, rp = e[a].detach().requires_grad_(), r[p].detach().requires_grad_()
        g = rng.standard_normal((N, E))
        out = sc.score_emb(ea, rp, e, "sp_") if direction == "sp_" else sc.score_emb(e, rp, ea, "_po")
        (out * torch.from_numpy(g)).sum().backward()
        ga, gm, gt = rr.pairs_bwd(direction, ent, rel, a, p, None, g)
        for got, want in ((ga, ea.grad), (gm, rp.grad), (gt, e.grad)):
            assert np.allclose(got[0], want.numpy(), rtol=1e-11, atol=1e-11), direction
    # the triple form: spo and both neg slots
    K = 3
    neg = rng.integers(0, E, (N, K))
    g = rng.standard_normal((N, K))
    for direction, a, slot in (("sp_", s, 2), ("_po", o, 0)):
        e = torch.from_numpy(ent).double()
        ea, rp, xr = e[a].clone().requires_grad_(), torch.from_numpy(rel).double()[p].requires_grad_(), \
            e[neg].clone().requires_grad_()
        tr = [None, rp.repeat_interleave(K, 0), None]
        tr[0 if slot == 2 else 2] = ea.repeat_interleave(K, 0)
        tr[slot] = xr.view(-1, D)
        (sc.score_emb(tr[0], tr[1], tr[2], "spo").view(N, K) * torch.from_numpy(g)).sum().backward()
        ga, gm, gx = rr.rows_bwd(direction, ent, rel, a, p, neg, g)
        for got, want in ((ga, ea.grad), (gm, rp.grad), (gx, xr.grad)):
            assert np.allclose(got[0], want.numpy(), rtol=1e-11, atol=1e-11), direction
    out, err = rr.accum([(np.array([1, 1, 2]), np.ones((3, 2)), np.zeros((3, 2)))], (4, 2))
    assert out[1, 0] == 2 and err[1, 0] == rr.U * 2 and err[2, 0] == 0


def test_committed_reference_outputs():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "rescal_scores_*.npz")))
    assert len(files) >= 2
    for f in files:
        z = np.load(f)
        ent, rel, s, p, o, sub = (z[k] for k in ("ent", "rel", "s", "p", "o", "sub"))
        assert ent.shape[0] <= 60 and ent.shape[1] <= 16
        for key, got in (("spo", rr.score_spo(ent, rel, s, p, o)), ("sp", rr.score_pairs("sp_", ent, rel, s, p)),
                         ("po", rr.score_pairs("_po", ent, rel, o, p)), ("sp_sub", rr.score_pairs("sp_", ent, rel, s, p, sub)),
                         ("po_sub", rr.score_pairs("_po", ent, rel, o, p, sub))):
            # the reference ran in float32: inside twice the bound (its own rounding and ours)
            assert (np.abs(z[key].astype(np.float64) - got[0]) <= 2 * rr.bound(got[1])).all(), (f, key)
        both = np.concatenate([z["sp_sub"], z["po_sub"]], 1)
        assert np.array_equal(z["sp_po_sub"], both)


@pytest.mark.parametrize("defect", ["sp_untransposed", "po_transposed", "outer_transposed", "last_coordinate"])
def test_planted_defects_exceed_the_bound(defect):
    ent, rel, s, p, o = _case(seed=9)
    d = D
    relT = rel.reshape(R, d, d).transpose(0, 2, 1).reshape(R, d * d)
    live = p != 1  # (the zero matrix hides everything)
    if "transposed" in defect:
        live = live & (p != 2)  # (and the identity its own transpose)
    if defect == "sp_untransposed":
        good, bad = rr.score_pairs("sp_", ent, rel, s, p), rr.score_pairs("sp_", ent, relT, s, p)[0]
    elif defect == "po_transposed":
        good, bad = rr.score_pairs("_po", ent, rel, o, p), rr.score_pairs("_po", ent, relT, o, p)[0]
    elif defect == "outer_transposed":
        g = np.random.default_rng(1).standard_normal((N, E))
        good = rr.pairs_bwd("sp_", ent, rel, s, p, None, g)[1]
        bad = good[0].reshape(N, d, d).transpose(0, 2, 1).reshape(N, d * d)
        live = np.ones(N, bool)
    else:
        good = rr.score_pairs("sp_", ent, rel, s, p)
        e2 = ent.copy()
        e2[:, -1] = 0
        bad = rr.score_pairs("sp_", e2, rel, s, p)[0]
    over = np.abs(bad - good[0]) > rr.bound(good[1])
    assert over[live].any(axis=1).all(), defect
