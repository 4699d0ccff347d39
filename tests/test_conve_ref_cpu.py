"""tests/_conve_ref.py and the package's torch route checked without a GPU: the restatement against the reference's
ConvEScorer.score_emb in eval mode (float64 torch), the torch route against the reference in train mode (both dropouts 0,
batch statistics on) and in eval mode with float64 autograd gradients, planted defects that must exceed 8x the bound on the
GPU cases' own inputs, and the shares that die and survive at each ReLU.

The tests that use only tests/_conve_ref.py and the reference (restatement against the reference, planted defects, ReLU
shares) validate the yardstick itself and pass without the feature; the torch-route, front-end and backward tests need
kge_amd.model.ConvEScorer and fail without it."""
import os
import sys

import numpy as np
import pytest
import torch

import _conve_ref as cr
from conftest import ROOT


def _reference_scorer(net, train=False):
    """the reference's ConvEScorer (kge/model/conve.py) in float64 with the parameters of `net`, built without a Config"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness as rh
    if not rh.available():
        pytest.skip("reference not on this machine")
    rh.import_reference()
    from kge.model.conve import ConvEScorer
    h, w, fs, pad = net["h"], net["w"], net["fs"], net["pad"]
    ref = ConvEScorer.__new__(ConvEScorer)
    torch.nn.Module.__init__(ref)
    ref.emb_dim, ref.emb_height, ref.emb_width = h * w, float(h), float(w)
    ref.filter_size, ref.stride, ref.padding = fs, 1, pad
    ref.feature_map_dropout, ref.projection_dropout = torch.nn.Dropout2d(0.0), torch.nn.Dropout(0.0)
    ref.convolution = torch.nn.Conv2d(1, 32, (fs, fs), stride=1, padding=pad, bias=net["conv_b"] is not None)
    ref.bn1 = torch.nn.BatchNorm2d(32, affine=False)
    ref.bn2 = torch.nn.BatchNorm1d(h * w, affine=False)
    ref.projection = torch.nn.Linear(net["proj_w"].shape[1], h * w)
    ref.non_linear = torch.nn.ReLU()
    ref.double()
    _load(ref, net)
    return ref.train(train)


def _load(sc, net):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    with torch.no_grad():
        sc.convolution.weight.copy_(t(net["conv_w"]).view_as(sc.convolution.weight))
        if net["conv_b"] is not None:
            sc.convolution.bias.copy_(t(net["conv_b"]))
        sc.bn1.running_mean.copy_(t(net["mean1"]))
        sc.bn1.running_var.copy_(t(net["var1"]))
        sc.bn2.running_mean.copy_(t(net["mean2"]))
        sc.bn2.running_var.copy_(t(net["var2"]))
        sc.projection.weight.copy_(t(net["proj_w"]))
        sc.projection.bias.copy_(t(net["proj_b"]))
    sc.bn1.eps, sc.bn2.eps = net["eps1"], net["eps2"]


def _front_end_scorer(net, train=False):
    from kge_amd import model
    sc = model.ConvEScorer(net["h"] * net["w"], aspect_ratio=net["w"] / net["h"], filter_size=net["fs"],
                           padding=net["pad"], feature_map_dropout=0.0, projection_dropout=0.0,
                           convolution_bias=net["conv_b"] is not None, dtype=torch.float64)
    assert (sc.emb_height, sc.emb_width) == (net["h"], net["w"])
    _load(sc, net)
    return sc.train(train)


@pytest.mark.parametrize("fs,pad", [(1, 0), (3, 0), (5, 0), (3, 1), (5, 2), (1, 2)])
@pytest.mark.parametrize("bias", [True, False])
def test_restatement_equals_the_reference_in_eval_mode(fs, pad, bias):
    net = cr.make_net(4, 8, fs, pad, bias, seed=fs + 10 * pad)
    ent, rel = cr.make_tables(9, 4, 32, 3)
    rng = np.random.default_rng(1)
    s, p, o = rng.integers(0, 9, 6), rng.integers(0, 4, 6), rng.integers(0, 9, 6)
    ref = _reference_scorer(net)
    e, r = torch.from_numpy(ent).double(), torch.from_numpy(rel).double()
    with torch.no_grad():
        want_sp = ref.score_emb(e[s], r[p], e, "sp_").numpy()
        want_spo = ref.score_emb(e[s], r[p], e[o], "spo").numpy().reshape(-1)
    got_sp, got_spo = cr.score_sp(net, ent, rel, s, p), cr.score_spo(net, ent, rel, s, p, o)
    assert np.allclose(got_sp[0], want_sp, rtol=1e-12, atol=1e-12)
    assert np.allclose(got_spo[0], want_spo, rtol=1e-12, atol=1e-12)
    assert (got_sp[1] > 0).all() and (got_sp[1] < 1e-2).all()
    sub = np.array([4, 0, 7])
    assert np.allclose(cr.score_sp(net, ent, rel, s, p, sub)[0], want_sp[:, sub], rtol=1e-12, atol=1e-12)
    q, eq = cr.queries(net, ent, rel, s, p)
    assert (q[:, 0] == 1).all() and not eq[:, 0].any()
    # the library-GEMM order is never tighter than the kernel's
    assert (cr.queries(net, ent, rel, s, p, order="any")[1] >= eq).all()


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("fs,pad,bias", [(3, 0, True), (5, 2, False), (1, 1, True)])
def test_torch_route_equals_the_reference(train, fs, pad, bias):
    """scores and float64 autograd gradients of every input and parameter; in train mode also the running statistics
    after the step"""
    net = cr.make_net(4, 8, fs, pad, bias, seed=3)
    ent, rel = cr.make_tables(9, 4, 32, 5)
    rng = np.random.default_rng(2)
    s, p, o = rng.integers(0, 9, 6), rng.integers(0, 4, 6), rng.integers(0, 9, 6)
    g = torch.from_numpy(rng.standard_normal((6, 9)))
    res = []
    for sc in (_reference_scorer(net, train), _front_end_scorer(net, train)):
        e, r = torch.from_numpy(ent).double().requires_grad_(), torch.from_numpy(rel).double().requires_grad_()
        sp = sc.score_emb(e[s], r[p], e, "sp_")
        spo = sc.score_emb(e[s], r[p], e[o], "spo")
        ((sp * g).sum() + (spo.view(-1) * g[:, 0]).sum()).backward()
        res.append([sp.detach(), spo.detach().view(-1), e.grad, r.grad] + [x.grad for x in sc.parameters()] +
                   [sc.bn1.running_mean, sc.bn1.running_var, sc.bn2.running_mean, sc.bn2.running_var])
        assert [k for k, _ in sc.named_parameters()] == (
            ["convolution.weight"] + (["convolution.bias"] if bias else []) + ["projection.weight", "projection.bias"])
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-10, atol=1e-10)
    assert res[0][2].abs().sum() > 0 and res[0][4].abs().sum() > 0


@pytest.mark.parametrize("name", ["seam", "default", "fs1_pad2_big_slice"])
def test_front_end_in_eval_mode_equals_the_restatement(name):
    net, ent, rel, s, p, o = cr.gpu_case(name)
    sc = _front_end_scorer(net)
    e, r = torch.from_numpy(ent).double(), torch.from_numpy(rel).double()
    with torch.no_grad():
        got = sc.score_emb(e[s], r[p], e, "sp_").numpy()
    assert np.allclose(got, cr.score_sp(net, ent, rel, s, p)[0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(cr.GPU_CASES))
def test_relu_shares_and_the_near_zero_variance(name):
    net, ent, rel, s, p, o = cr.gpu_case(name)
    dead1, dead2 = cr.shares(net, ent, rel, s, p)
    assert 0.2 < dead1 < 0.8 and 0.2 < dead2 < 0.8, "some features and some outputs die at each ReLU, some survive"
    assert net["var1"].min() < 1e-6 < net["eps1"] * 10, "one running variance near 0"
    assert s[0] == s[-1] and p[0] == p[-1]


@pytest.mark.parametrize("defect", cr.DEFECTS)
def test_planted_defects_exceed_eight_times_the_bound(defect):
    for name in cr.GPU_CASES:
        net, ent, rel, s, p, o = cr.gpu_case(name)
        if defect == "flipped_taps" and net["fs"] == 1:
            continue  # (one tap has no order)
        good, e = cr.score_sp(net, ent, rel, s, p)
        bad = cr.score_sp(net, ent, rel, s, p, defect=defect)[0]
        over = np.abs(bad - good) > 8 * cr.bound(e)
        assert over.any(axis=1).mean() > 0.5, (defect, name)
        gq, eq = cr.queries(net, ent, rel, s, p)
        if defect not in ("bias_from_the_end",):
            bq = cr.queries(net, ent, rel, s, p, defect=defect)[0]
            assert (np.abs(bq - gq) > 8 * cr.bound(eq)).any(), (defect, name, "on the query rows")


@pytest.mark.parametrize("name", ["seam", "seam_no_bias"])
def test_backward_restatement_equals_autograd_of_the_front_end(name):
    """tests/_conve_bwd_ref.py: its float64 gradients equal float64 autograd through the package's ConvEScorer, its
    bound is positive wherever a gradient can be non-zero, and the cases' ReLU masks are stable"""
    import _conve_bwd_ref as br
    from kge_amd import model
    net, ent, rel, s, p, o = cr.gpu_case(name)
    rng = np.random.default_rng(4)
    G, g = rng.standard_normal((len(s), ent.shape[0])), rng.standard_normal(len(s))
    ref, stable = br.gradients(net, ent, rel, s, p, o, G, g)
    assert stable
    sc = model.ConvEScorer.__new__(model.ConvEScorer)
    torch.nn.Module.__init__(sc)
    h, w, fs = net["h"], net["w"], net["fs"]
    sc.emb_height, sc.emb_width, sc.emb_dim, sc.filter_size, sc.stride, sc.padding = h, w, h * w, fs, 1, net["pad"]
    sc.feature_map_dropout, sc.projection_dropout = torch.nn.Dropout2d(0.0), torch.nn.Dropout(0.0)
    sc.convolution = torch.nn.Conv2d(1, 32, (fs, fs), padding=net["pad"], bias=net["conv_b"] is not None)
    sc.bn1, sc.bn2 = torch.nn.BatchNorm2d(32, affine=False), torch.nn.BatchNorm1d(h * w, affine=False)
    sc.projection = torch.nn.Linear(net["proj_w"].shape[1], h * w)
    sc.double()
    _load(sc, net)
    sc.eval()
    e, r = torch.from_numpy(ent).double().requires_grad_(), torch.from_numpy(rel).double().requires_grad_()
    loss = (sc.score_emb(e[s], r[p], e, "sp_") * torch.from_numpy(G)).sum() + \
        (sc.score_emb(e[s], r[p], e[o], "spo").view(-1) * torch.from_numpy(g)).sum()
    loss.backward()
    got = dict(ent=e.grad, rel=r.grad, conv_w=sc.convolution.weight.grad, proj_w=sc.projection.weight.grad,
               proj_b=sc.projection.bias.grad)
    if net["conv_b"] is not None:
        got["conv_b"] = sc.convolution.bias.grad
    assert set(got) == set(ref)
    for k, (want, tol) in ref.items():
        assert np.allclose(got[k].numpy().reshape(want.shape), want, rtol=1e-10, atol=1e-10), k
        assert (tol > 0).all() and (tol[np.abs(want) > 0] < 1e-1 * np.abs(want).max() + 1e-3).all(), k


@pytest.mark.parametrize("fs,pad,bias", [(3, 0, True), (3, 1, False)])
def test_training_mode_restatement_and_its_bound(fs, pad, bias):
    """tests/_conve_train_ref.py: scores and gradients equal float64 autograd through the package's ConvEScorer in
    training mode (batch statistics, dropouts 0); a float32 evaluation of the same scorer on the CPU lies inside the
    bound; the true gradient of convolution.bias is 0 under batch statistics"""
    import _conve_train_ref as tr
    net = cr.make_net(2, 4, fs, pad, bias, seed=5)
    ent, rel = cr.make_tables(30, 6, 8, 9)
    rng = np.random.default_rng(3)
    n = 48
    s, p = rng.integers(0, 30, n), rng.integers(0, 6, n)
    G = rng.standard_normal((n, 30)) / n
    P = dict(ent=ent, rel=rel, conv_w=net["conv_w"].reshape(32, 1, fs, fs), conv_b=net["conv_b"], proj_w=net["proj_w"],
             proj_b=net["proj_b"])
    scores, sb, grads, unstable = tr.node(P, 2, 4, pad, 1e-5, 1e-5, s, p, G)
    for dtype, exact in ((torch.float64, True), (torch.float32, False)):
        sc = _front_end_scorer(net, train=True).to(dtype)
        e = torch.from_numpy(ent).to(dtype).requires_grad_()
        r = torch.from_numpy(rel).to(dtype).requires_grad_()
        out = sc.score_emb(e[s], r[p], e, "sp_")
        (out * torch.from_numpy(G).to(dtype)).sum().backward()
        got = dict(ent=e.grad, rel=r.grad, conv_w=sc.convolution.weight.grad, proj_w=sc.projection.weight.grad,
                   proj_b=sc.projection.bias.grad)
        if bias:
            got["conv_b"] = sc.convolution.bias.grad
        assert set(got) == set(grads)
        if exact:
            assert np.allclose(out.detach().numpy(), scores, rtol=1e-10, atol=1e-10)
        else:
            assert (np.abs(out.detach().double().numpy() - scores) <= sb).all()
        for k, (want, tol) in grads.items():
            g = got[k].double().numpy().reshape(want.shape)
            if exact:
                assert np.allclose(g, want, rtol=1e-9, atol=1e-9), k
            else:
                assert (np.abs(g - want) <= tol).all(), (k, float((np.abs(g - want) / tol).max()))
    if bias:
        assert np.abs(grads["conv_b"][0]).max() < 1e-12 and (grads["conv_b"][1] > 0).all()
    assert np.abs(grads["proj_b"][0]).max() < 1e-12 and (grads["proj_b"][1] > 0).all()
    assert (sb > 0).all()
    assert (np.abs(scores) > sb).mean() > 0.9, "the scores' bound is far below the scores"
