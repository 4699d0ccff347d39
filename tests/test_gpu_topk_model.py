"""KgeModel.predict_o / predict_s on the GPU: the fused route (kge_topk with the ranges of a device-resident
FilterIndex) against the numpy restatement on the model's own score_sp / score_po, and against the same model's torch
composition (the route a model takes when the fused one does not apply) wherever the two score matrices agree bit for
bit."""
import numpy as np
import pytest
import torch

import _topk_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, R, D, N = 1500, 7, 64, 70


@pytest.fixture(scope="module")
def split():
    from kge_amd.eval import FilterIndex
    from kge_amd.synthetic import make_splits
    ds = make_splits(E, R, 20000, 300, 300, seed=1)
    fi = FilterIndex([ds["train"], ds["valid"]], E, R)
    tri = torch.from_numpy(ds["valid"][:N].astype(np.int64))
    return fi, tri


def _model(name, integer=False):
    from kge_amd import model as M
    torch.manual_seed(3)
    mdl = M.create(name, E, R, D, device=DEV)
    if integer:
        with torch.no_grad():
            for emb in (mdl._entity_embedder, mdl._relation_embedder):
                emb._embeddings.weight.copy_(torch.randint(-2, 3, emb._embeddings.weight.shape, device=DEV).float())
    return mdl.eval()


def _check(got, want):
    val, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(idx, want[1])
    assert np.array_equal(val.view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("name", ["complex", "distmult", "transe", "rotate"])
def test_predict_equals_the_restatement_on_the_models_scores(name, split):
    fi, tri = split
    mdl = _model(name)
    s, p, o = (tri[:, j].to(DEV) for j in range(3))
    sb, se, pb, pe = fi.ranges(tri.numpy())
    assert (se - sb).max() > 1 and (pe - pb).max() > 1  # rows with several known answers
    with torch.no_grad():
        sc_sp = mdl.score_sp(s, p).cpu().numpy()
        sc_po = mdl.score_po(p, o).cpu().numpy()
    for k in (1, 10, 128):
        _check(mdl.predict_o(s, p, k, fi, o), ref.topk_ref(sc_sp, k, [(sb, se, fi.sp_values)], tri[:, 2].numpy()))
        _check(mdl.predict_s(p, o, k, fi, s), ref.topk_ref(sc_po, k, [(pb, pe, fi.po_values)], tri[:, 0].numpy()))
    _check(mdl.predict_o(s, p, 10, fi), ref.topk_ref(sc_sp, 10, [(sb, se, fi.sp_values)]))   # the true object filtered too
    _check(mdl.predict_s(p, o, 10), ref.topk_ref(sc_po, 10))                                 # no filter index
    assert set(fi.__dict__["_predict_arrays"]) == {(DEV, "sp"), (DEV, "po")}                 # cached on the index object


@pytest.mark.parametrize("name,integer", [("distmult", True), ("transe", True), ("complex", False), ("rotate", False)])
def test_fused_route_equals_the_torch_composition_where_the_scores_agree(name, integer, split, monkeypatch):
    """The composition scores with a model on CPU-side torch arithmetic (one float32 sum per score in torch's order);
    on small-integer tables every sum is exact, so DistMult's matrices agree everywhere."""
    from kge_amd import model as M
    fi, tri = split
    mdl = _model(name, integer)
    s, p, o = (tri[:, j].to(DEV) for j in range(3))
    with torch.no_grad():
        fused_sp, fused_po = mdl.score_sp(s, p).cpu(), mdl.score_po(p, o).cpu()
        ent, rel = mdl._entity_embedder.weight.cpu(), mdl._relation_embedder.weight.cpu()
    torch_sp, torch_po = _torch_scores(name, ent, rel, tri, mdl._scorer._norm)
    same_sp = (fused_sp.view(torch.int32) == torch_sp.view(torch.int32)).all(dim=1).numpy()
    same_po = (fused_po.view(torch.int32) == torch_po.view(torch.int32)).all(dim=1).numpy()
    if name == "distmult":
        assert same_sp.all() and same_po.all()
    k = 10
    got_o, got_s = mdl.predict_o(s, p, k, fi, o), mdl.predict_s(p, o, k, fi, s)
    # the composed route of the same model: fused off, its score calls answered with the torch matrices
    monkeypatch.setattr(mdl, "_fused", lambda: False)
    monkeypatch.setattr(mdl, "score_sp", lambda s_, p_, o_=None: torch_sp.to(DEV))
    monkeypatch.setattr(mdl, "score_po", lambda p_, o_, s_=None: torch_po.to(DEV))
    comp_o, comp_s = mdl.predict_o(s, p, k, fi, o), mdl.predict_s(p, o, k, fi, s)
    assert np.array_equal(got_o[1].cpu().numpy()[same_sp], comp_o[1].cpu().numpy()[same_sp])
    assert np.array_equal(got_s[1].cpu().numpy()[same_po], comp_s[1].cpu().numpy()[same_po])


def _torch_scores(name, ent, rel, tri, l_norm):
    """score_sp / score_po [n, E] in plain torch on the CPU (the reference scorers' formulas)."""
    s, p, o = ent[tri[:, 0]], rel[tri[:, 1]], ent[tri[:, 2]]
    if name == "distmult":
        return (s * p) @ ent.t(), (o * p) @ ent.t()
    if name == "transe":
        return -torch.cdist(s + p, ent, p=l_norm), -torch.cdist(o - p, ent, p=l_norm)
    h = ent.shape[1] // 2
    if name == "complex":
        sr, si, pr, pi, orr, oi = s[:, :h], s[:, h:], p[:, :h], p[:, h:], o[:, :h], o[:, h:]
        q_sp = torch.cat((sr * pr - si * pi, sr * pi + si * pr), dim=1)
        q_po = torch.cat((pr * orr + pi * oi, pr * oi - pi * orr), dim=1)
        return q_sp @ ent.t(), q_po @ ent.t()
    # rotate: || s o e^{i p} - o ||
    c, sn = torch.cos(p), torch.sin(p)
    sr, si, orr, oi = s[:, :h], s[:, h:], o[:, :h], o[:, h:]
    fr, fi_ = sr * c - si * sn, sr * sn + si * c          # s rotated forward
    br, bi = orr * c + oi * sn, oi * c - orr * sn         # o rotated backward
    er, ei = ent[:, :h], ent[:, h:]

    def dist(qr, qi):
        return -torch.sqrt((qr[:, None, :] - er[None]) ** 2 + (qi[:, None, :] - ei[None]) ** 2).sum(dim=2)
    return dist(fr, fi_), dist(br, bi)
