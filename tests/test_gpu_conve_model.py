"""model.create("conve", ...) on the GPU: score_sp / score_spo against the derived bound of tests/_conve_ref.py on both
routes, which route ran (the model's own counters), the padded-table cache and its invalidation by an optimizer step, the
state_dict round trip, and the declined calls."""
import numpy as np
import pytest
import torch

import _conve_ref as cr

pytestmark = pytest.mark.gpu

E, R = cr.GPU_E, cr.GPU_R


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


def _model(name, dev, **kw):
    """the model of a named case of _conve_ref.GPU_CASES (aspect ratio 2 only), parameters and statistics loaded"""
    from kge_amd import model
    net, ent, rel, s, p, o = cr.gpu_case(name)
    m = model.create("conve", E, R, net["h"] * net["w"], filter_size=net["fs"], padding=net["pad"],
                     convolution_bias=net["conv_b"] is not None, device=dev, **kw)
    sc = m.get_scorer()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    with torch.no_grad():
        m.get_s_embedder().weight.copy_(t(ent))
        m.get_p_embedder().weight.copy_(t(rel))
        sc.convolution.weight.copy_(t(net["conv_w"]).view_as(sc.convolution.weight))
        if net["conv_b"] is not None:
            sc.convolution.bias.copy_(t(net["conv_b"]))
        sc.projection.weight.copy_(t(net["proj_w"]))
        sc.projection.bias.copy_(t(net["proj_b"]))
        for bn, mk, vk in ((sc.bn1, "mean1", "var1"), (sc.bn2, "mean2", "var2")):
            bn.running_mean.copy_(t(net[mk]))
            bn.running_var.copy_(t(net[vk]))
    ix = [torch.from_numpy(x).to(dev) for x in (s, p, o)]
    return m.eval(), net, ent, rel, (s, p, o), ix


def _within(got, ref, what):
    want, e = ref
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    err, tol = np.abs(got - want), cr.bound(e)
    print("{}: max err / bound = {:.4f}".format(what, float((err / tol).max())))
    assert (err <= tol).all(), what


@pytest.mark.parametrize("name", ["seam", "default", "fs1_pad2_big_slice", "seam_no_bias"])
def test_scores_on_both_routes_and_which_route_ran(dev, name):
    m, net, ent, rel, (s, p, o), (st, pt, ot) = _model(name, dev)
    sub = np.array([3, 0, 22, 7])
    refs = {order: (cr.score_sp(net, ent, rel, s, p, order=order), cr.score_spo(net, ent, rel, s, p, o, order=order),
                    cr.score_sp(net, ent, rel, s, p, sub, order=order)) for order in ("kernel", "any")}
    with torch.no_grad():
        assert m.kernel_route()
        sp, spo, sps = m.score_sp(st, pt), m.score_spo(st, pt, ot, "o"), m.score_sp(st, pt, torch.from_numpy(sub).to(dev))
    assert m.routes == {"kernel": 3, "torch": 0} and m.paddings == 1
    assert tuple(sp.shape) == (len(s), E) and tuple(spo.shape) == (len(s),) and tuple(sps.shape) == (len(s), 4)
    for got, ref, what in zip((sp, spo, sps), refs["kernel"], ("sp_", "spo", "sp_ subset")):
        _within(got, ref, "{} kernel route {}".format(name, what))
    # a recorded gradient: the torch route in eval mode (library convolution and GEMM: a sum in any order)
    assert not m.kernel_route()
    sp2, spo2 = m.score_sp(st, pt), m.score_spo(st, pt, ot, "o")
    assert m.routes == {"kernel": 3, "torch": 2} and sp2.requires_grad
    _within(sp2, refs["any"][0], name + " torch route sp_")
    _within(spo2, refs["any"][1], name + " torch route spo")
    (sp2.sum() + spo2.sum()).backward()
    for prm in m.parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and bool(prm.grad.abs().sum() > 0)
    # equal rows of a batch, equal scores; the batch shape does not move a bit on the kernel route
    with torch.no_grad():
        assert torch.equal(sp[0], sp[-1])
        for n in (1, 7, 33):
            assert torch.equal(m.score_sp(st[:n], pt[:n]), sp[:n])
            assert torch.equal(m.score_spo(st[:n], pt[:n], ot[:n], "o"), spo[:n])


def test_training_mode_takes_the_torch_route_and_updates_the_statistics(dev):
    m, net, ent, rel, (s, p, o), (st, pt, ot) = _model("seam", dev, feature_map_dropout=0.0, projection_dropout=0.0)
    m.train()
    before = m.get_scorer().bn1.running_mean.clone()
    out = m.score_sp(st, pt)
    assert m.routes == {"kernel": 0, "torch": 1} and out.requires_grad
    assert not torch.equal(m.get_scorer().bn1.running_mean, before), "batch statistics on"
    with torch.no_grad():
        m.score_sp(st, pt)
    assert m.routes["kernel"] == 0, "training mode never takes the kernel route"


def test_cache_invalidation_after_an_optimizer_step_and_the_byte_cap(dev):
    m, net, ent, rel, (s, p, o), (st, pt, ot) = _model("seam", dev)
    with torch.no_grad():
        a = m.score_sp(st, pt)
        m.score_sp(st, pt)
    assert m.paddings == 1, "one padded copy per version of the entity table"
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    m.score_sp(st, pt).sum().backward()
    opt.step()
    with torch.no_grad():
        b = m.score_sp(st, pt)
    assert m.paddings == 2 and not torch.equal(a, b)
    ent2 = m.get_s_embedder().weight.detach().cpu().numpy()
    rel2 = m.get_p_embedder().weight.detach().cpu().numpy()
    sc = m.get_scorer()
    net2 = dict(net, conv_w=sc.convolution.weight.detach().cpu().numpy().reshape(32, net["fs"], net["fs"]),
                conv_b=sc.convolution.bias.detach().cpu().numpy(), proj_w=sc.projection.weight.detach().cpu().numpy(),
                proj_b=sc.projection.bias.detach().cpu().numpy())
    _within(b, cr.score_sp(net2, ent2, rel2, s, p), "after the step")
    # above the cap: no copy, the plain rows, the same scores inside the bound
    m.padded_table_max_bytes = 16
    with torch.no_grad():
        c = m.score_sp(st, pt)
    assert m.paddings == 2 and m.padded_table() is None
    _within(c, cr.score_sp(net2, ent2, rel2, s, p), "without the padded copy")


def test_state_dict_round_trip_and_declined_calls(dev):
    from kge_amd import model
    m, net, ent, rel, (s, p, o), (st, pt, ot) = _model("seam", dev)
    sd = m.state_dict()
    assert {"_scorer.convolution.weight", "_scorer.bn1.running_var", "_scorer.bn2.running_mean",
            "_scorer.projection.bias", "_entity_embedder._embeddings.weight"} <= set(sd)
    m2 = model.create("conve", E, R, 8, device=dev).eval()
    m2.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(m2.score_sp(st, pt), m.score_sp(st, pt))
    z = st[:2]
    with pytest.raises(ValueError, match="ConvE can only score objects"):
        m.score_spo(z, z, z, "s")
    with pytest.raises(Exception, match="Combine _po not supported"):
        m.score_po(z, z)
    with pytest.raises(ValueError, match="negative-sampling blocks"):
        m.score_neg(z, z, z, 2, z.view(2, 1))
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(1), torch.zeros(1)))
    with pytest.raises(ValueError, match="kge_tables"):
        m.tables()
    vals, ids = m.predict_o(st, pt, 3)
    with torch.no_grad():
        want = m.score_sp(st, pt)
    assert torch.equal(vals[:, 0], want.max(1).values)


@pytest.mark.parametrize("name", ["seam", "seam_no_bias"])
def test_torch_route_gradients_within_the_backward_bound(dev, name):
    """the gradients of the entity and relation tables, the convolution and the projection on the torch route in eval
    mode (_ScoreEmb over q' = [1 | x]: kge_score_emb_bwd, the dropped column 0, the bias column of the entity gradient)
    against float64 autograd of the restatement, inside the bound of tests/_conve_bwd_ref.py"""
    import _conve_bwd_ref as br
    m, net, ent, rel, (s, p, o), (st, pt, ot) = _model(name, dev)
    rng = np.random.default_rng(4)
    G, g = rng.standard_normal((len(s), E)).astype(np.float32), rng.standard_normal(len(s)).astype(np.float32)
    ref, stable = br.gradients(net, ent, rel, s, p, o, G, g)
    assert stable, "every pre-activation is farther from 0 than its forward bound: the ReLU masks are the same"
    sp, spo = m.score_sp(st, pt), m.score_spo(st, pt, ot, "o")
    assert m.routes == {"kernel": 0, "torch": 2}
    ((sp * torch.from_numpy(G).to(dev)).sum() + (spo * torch.from_numpy(g).to(dev)).sum()).backward()
    sc = m.get_scorer()
    got = dict(ent=m.get_s_embedder().weight.grad, rel=m.get_p_embedder().weight.grad, conv_w=sc.convolution.weight.grad,
               proj_w=sc.projection.weight.grad, proj_b=sc.projection.bias.grad)
    if net["conv_b"] is not None:
        got["conv_b"] = sc.convolution.bias.grad
    assert set(got) == set(ref)
    for k, (want, tol) in ref.items():
        err = np.abs(got[k].double().cpu().numpy().reshape(want.shape) - want)
        print("{} gradient of {}: max err / bound = {:.4f}".format(name, k, float((err / tol).max())))
        assert (err <= tol).all(), k
        assert np.abs(want).sum() > 0
    assert np.abs(ref["ent"][0][:, 0]).sum() > 0 and not ref["rel"][0][:, 0].any(), "bias column; relation column 0 unused"
    assert not bool(got["rel"][:, 0].any())
