"""tests/_tucker3_ref.py checked without a GPU: against the imported reference model, against float64 autograd for g_B and
g_W, against committed outputs of the reference model (tests/golden/tucker3_scores_*.npz), and by planted defects that
must exceed the bound.

These are tests of the RESTATEMENT, the yardstick of the GPU tests: apart from the committed goldens they use no code of
the package, so they pass with or without the Tucker3 kernels.  The tests that need the feature are
test_abi_tucker3_cpu.py and the test_gpu_*tucker3* files."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

import _tucker3_ref as tr
from conftest import ROOT

E, R, D, DR, N = 11, 4, 6, 5, 7


def _case(seed=3):
    ent, B, W = tr.make_params(E, R, D, DR, seed)
    rng = np.random.default_rng(seed)
    s, p, o = rng.integers(0, E, N), rng.integers(0, R, N), rng.integers(0, E, N)
    p[:3] = [1, 2, 2]
    return ent, B, W, s, p, o


def _torch_scores(ent, B, W, s, p, o):
    """the reference's operation sequence in float64 torch: F.linear, view(d, d), s^T M o"""
    e = torch.from_numpy(ent).double()
    M = torch.nn.functional.linear(B[p], W).view(-1, D, D)
    sp = torch.einsum("na,nab,mb->nm", e[s], M, e)
    po = torch.einsum("ma,nab,nb->nm", e, M, e[o])
    spo = torch.einsum("na,nab,nb->n", e[s], M, e[o])
    return spo, sp, po


def test_restatement_equals_the_operation_sequence_and_its_autograd():
    ent, B, W, s, p, o = _case()
    Bt, Wt = (torch.from_numpy(x).double().requires_grad_() for x in (B, W))
    spo, sp, po = _torch_scores(ent, Bt, Wt, s, p, o)
    M, eM = tr.project(B, W, p)
    assert (eM[p == 1] == 0).all() and not M[p == 1].any(), "the zero base row: exactly zero, zero bound"
    for got, want in ((tr.score_spo(ent, M, eM, s, o), spo), (tr.score_pairs("sp_", ent, M, eM, s), sp),
                      (tr.score_pairs("_po", ent, M, eM, o), po)):
        assert np.allclose(got[0], want.detach().numpy(), rtol=1e-12, atol=1e-12)
        assert (got[1] >= 0).all() and (got[1] > 0).any() and (got[1] < 1e-3).all()
    rng = np.random.default_rng(5)
    g = rng.standard_normal((N, E))
    (sp * torch.from_numpy(g)).sum().backward()
    _, gm, _ = tr.pairs_bwd("sp_", ent, M, eM, s, None, g)
    (rows, e_rows), (g_w, e_w) = tr.project_bwd(B, W, p, *gm)
    g_b, e_b = tr.base_grad(R, p, rows, e_rows)
    assert np.allclose(g_b, Bt.grad.numpy(), rtol=1e-11, atol=1e-11) and np.allclose(g_w, Wt.grad.numpy(), rtol=1e-11, atol=1e-11)
    # the "all" route: the table's gradient first, then the projection backward over all rows -- the same values
    GM, eGM = tr.table_grad(R, p, *gm)
    (rows2, _), (g_w2, _) = tr.project_bwd(B, W, None, GM, eGM)
    assert np.allclose(rows2, g_b, rtol=1e-11, atol=1e-11) and np.allclose(g_w2, g_w, rtol=1e-11, atol=1e-11)
    assert (e_b >= 0).all() and (e_w > 0).any()


def _reference():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness as rh
    if not rh.available():
        pytest.skip("reference not on this machine")
    return rh


def test_restatement_against_the_imported_reference_model():
    rh = _reference()
    torch.manual_seed(7)
    m = rh.make_model("relational_tucker3", 37, 5, 8, options={"relational_tucker3.entity_embedder.dim": 8,
                                                               "relational_tucker3.relation_embedder.base_embedder.dim": 5})
    sd = m.state_dict()
    assert set(sd) == {"_entity_embedder._embeddings.weight", "_relation_embedder.base_embedder._embeddings.weight",
                       "_relation_embedder.projection.weight"}
    ent, B, W = (sd[k].numpy() for k in ("_entity_embedder._embeddings.weight",
                                         "_relation_embedder.base_embedder._embeddings.weight",
                                         "_relation_embedder.projection.weight"))
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (9,), generator=g) for hi in (37, 5, 37))
    M, eM = tr.project(B, W, p.numpy())
    with torch.no_grad():  # float32 torch: its own rounding, inside the same bound
        for got, ref in ((m.score_spo(s, p, o, "o"), tr.score_spo(ent, M, eM, s.numpy(), o.numpy())),
                         (m.score_sp(s, p), tr.score_pairs("sp_", ent, M, eM, s.numpy())),
                         (m.score_po(p, o), tr.score_pairs("_po", ent, M, eM, o.numpy()))):
            assert (np.abs(got.double().numpy().reshape(ref[0].shape) - ref[0]) <= tr.bound(ref[1])).all()


def test_committed_reference_outputs():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "tucker3_scores_*.npz")))
    assert len(files) == 2
    for f in files:
        z = np.load(f)
        ent, B, W, s, p, o, sub = (z[k] for k in ("ent", "base", "proj", "s", "p", "o", "sub"))
        M, eM = tr.project(B, W, p)
        m = len(sub)
        refs = {"spo": tr.score_spo(ent, M, eM, s, o), "sp": tr.score_pairs("sp_", ent, M, eM, s),
                "po": tr.score_pairs("_po", ent, M, eM, o), "sp_sub": tr.score_pairs("sp_", ent, M, eM, s, sub),
                "po_sub": tr.score_pairs("_po", ent, M, eM, o, sub)}
        for k, (want, e) in refs.items():
            assert (np.abs(z[k].astype(np.float64).reshape(want.shape) - want) <= tr.bound(e)).all(), (f, k)
        both = z["sp_po_sub"].astype(np.float64)
        assert (np.abs(both[:, :m] - refs["sp_sub"][0]) <= tr.bound(refs["sp_sub"][1])).all()
        assert (np.abs(both[:, m:] - refs["po_sub"][0]) <= tr.bound(refs["po_sub"][1])).all()


def test_planted_defects_exceed_the_bound():
    ent, B, W, s, p, o = _case()
    M, eM = tr.project(B, W, p)
    sp, e_sp = tr.score_pairs("sp_", ent, M, eM, s)
    live = p != 1  # (the zero base row hides every defect of the projection)

    def exceeds(M_bad):
        bad = tr.score_pairs("sp_", ent, M_bad, eM, s)[0]
        return (np.abs(bad - sp) > tr.bound(e_sp))[live].any()

    # W read as [d_r, d^2]
    Wt = np.ascontiguousarray(W.reshape(DR, D * D).T)
    assert exceeds(tr.project(B, Wt, p)[0])
    # M transposed
    assert exceeds(M.reshape(-1, D, D).transpose(0, 2, 1).reshape(-1, D * D))
    # the last k dropped
    assert exceeds(tr.project(B[:, :-1], W[:, :-1], p)[0])
    assert (np.abs(tr.project(B[:, :-1], W[:, :-1], p)[0] - M) > tr.bound(eM))[live].any()
    # a gradient scattered to the wrong base row
    g = np.random.default_rng(9).standard_normal((N, E))
    _, gm, _ = tr.pairs_bwd("sp_", ent, M, eM, s, None, g)
    (rows, e_rows), _ = tr.project_bwd(B, W, p, *gm)
    g_b, e_b = tr.base_grad(R, p, rows, e_rows)
    wrong = p.copy()
    wrong[-1] = (wrong[-1] + 1) % R
    bad, _ = tr.base_grad(R, wrong, rows, e_rows)
    assert (np.abs(bad - g_b) > tr.bound(e_b)).any()
