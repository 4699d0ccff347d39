"""The ConvE entries of the C ABI without a GPU: symbols and signatures, the struct layout, every status code of the gate
reached without a launch (with kge_conve_workspace_bytes returning 0), n == 0, and the front end's refusals and route rule
on CPU tensors."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("kge_conve_workspace_bytes", "kge_conve_queries")
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    return _lib.lib()


def _net(**kw):
    from kge_amd import _lib
    v = dict(h=3, w=5, filter_size=3, padding=0, has_conv_bias=1, reserved_=0, conv_w=16, conv_b=16, bn1_mean=16,
             bn1_var=16, proj_w=16, proj_ld=None, proj_b=16, bn2_mean=16, bn2_var=16, bn1_eps=1e-5, bn2_eps=1e-5)
    v.update(kw)
    if v["proj_ld"] is None:
        v["proj_ld"] = max(32 * (2 * v["h"] - v["filter_size"] + 2 * v["padding"] + 1) *
                           (v["w"] - v["filter_size"] + 2 * v["padding"] + 1), 1)
    return _lib.KgeConveNet(**v)


def _ix(ptr=16, itype=1, start=0, stride=1):
    from kge_amd import _lib
    return _lib.KgeIndex(ptr, itype, start, stride)


def _call(lib, c, n=3, **kw):
    d = c.h * c.w
    a = dict(ent=16, ent_ld=d + 1, rel=16, rel_ld=d + 1, s=_ix(), p=_ix(), q=16, q_ld=d + 1, ws=16, ws_bytes=1 << 40)
    a.update(kw)
    return lib.kge_conve_queries(ctypes.byref(c), a["ent"], a["ent_ld"], a["rel"], a["rel_ld"], a["s"], a["p"], n, a["q"],
                                 a["q_ld"], a["ws"], a["ws_bytes"], None)


def test_symbols_signatures_and_struct_layout(lib):
    from kge_amd import _lib
    header = open(ROOT + "/include/kge_amd.h").read()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\(", header), name
    assert "conve.py:75-93" in header
    for macro, val in (("KGE_CONVE_MAX_DIM", _lib.CONVE_MAX_DIM), ("KGE_CONVE_MAX_SLICE", _lib.CONVE_MAX_SLICE)):
        assert int(re.search(r"#define " + macro + r" (\d+)", header).group(1)) == val
    fields = re.search(r"typedef struct kge_conve_net \{(.*?)\} kge_conve_net;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+);", fields)
    assert names == [f[0] for f in _lib.KgeConveNet._fields_]
    assert ctypes.sizeof(_lib.KgeConveNet) == 6 * 4 + 9 * 8 + 2 * 4 == 104
    assert _lib.KgeConveNet.conv_w.offset == 24 and _lib.KgeConveNet.proj_ld.offset == 64
    assert _lib.KgeConveNet.bn1_eps.offset == 96 and _lib.KgeConveNet.bn2_eps.offset == 100
    assert _lib.PROTOTYPES["kge_conve_queries"][0] is ctypes.c_int and len(_lib.PROTOTYPES["kge_conve_queries"][1]) == 13


def test_the_gate_rejects_before_any_launch(lib):
    n = 3
    unsupported = (_net(filter_size=0), _net(filter_size=6, h=4, w=8), _net(padding=3),
                   _net(h=1, w=2, filter_size=3),                  # Ho = 0
                   _net(h=4, w=2, filter_size=3),                  # Wo = 0
                   _net(h=25, w=41),                               # h * w = 1025
                   _net(h=20, w=40, filter_size=1, padding=2))     # a slice of 44 x 44 positions: 1937 floats a row
    for c in unsupported:
        assert _call(lib, c, n) == UNSUPPORTED
        assert lib.kge_conve_workspace_bytes(ctypes.byref(c), n) == 0
    invalid = (_net(h=0), _net(w=0), _net(padding=-1), _net(proj_ld=32 * 4 * 3 - 1), _net(conv_w=None),
               _net(conv_b=None), _net(bn1_mean=None), _net(bn1_var=None), _net(proj_w=None), _net(proj_b=None),
               _net(bn2_mean=None), _net(bn2_var=None))
    for c in invalid:
        assert _call(lib, c, n) == INVALID
    assert lib.kge_conve_workspace_bytes(ctypes.byref(_net(proj_ld=1)), n) == 0
    assert lib.kge_conve_workspace_bytes(None, n) == 0
    assert lib.kge_conve_queries(None, 16, 16, 16, 16, _ix(), _ix(), n, 16, 16, 16, 1 << 30, None) == INVALID
    c = _net()
    assert lib.kge_conve_workspace_bytes(ctypes.byref(c), n) == 32 * n * 15 * 4
    assert lib.kge_conve_workspace_bytes(ctypes.byref(c), 0) == 0 and lib.kge_conve_workspace_bytes(ctypes.byref(c), -1) == 0
    # a bias that is not used may be NULL; the largest shapes inside the gate pass
    assert lib.kge_conve_workspace_bytes(ctypes.byref(_net(has_conv_bias=0, conv_b=None)), 1) > 0
    assert _call(lib, _net(has_conv_bias=0, conv_b=None), 0) == OK
    assert lib.kge_conve_workspace_bytes(ctypes.byref(_net(h=10, w=20, filter_size=1, padding=2)), 1) == 32 * 200 * 4
    assert lib.kge_conve_workspace_bytes(ctypes.byref(_net(h=16, w=32, filter_size=5, padding=0)), 1) > 0  # 28 x 28
    # malformed calls
    for kw in (dict(ent_ld=15), dict(rel_ld=15), dict(q_ld=15), dict(q=None), dict(ent=None), dict(rel=None),
               dict(s=_ix(itype=5)), dict(p=_ix(stride=0)), dict(s=_ix(start=1)), dict(p=_ix(ptr=None, start=-1))):
        assert _call(lib, c, n, **kw) == INVALID, kw
    assert _call(lib, c, -1) == INVALID
    assert _call(lib, c, n, ws=None) == WORKSPACE and _call(lib, c, n, ws_bytes=32 * n * 15 * 4 - 1) == WORKSPACE
    # an argument error is reported in front of an unsupported shape
    assert _call(lib, _net(padding=3), n, q_ld=3) == INVALID


def test_empty_calls_launch_nothing(lib):
    c = _net()
    assert _call(lib, c, 0, q=None, ws=None, ws_bytes=0) == OK
    assert _call(lib, c, 0, ent=None, rel=None, q=None, ws=None, ws_bytes=0) == OK


def test_model_shape_rule_refusals_and_route_on_cpu_tensors():
    from kge_amd import engine, model
    assert model.conve_image_shape(200) == (10, 20, 200)
    assert model.conve_image_shape(190, 2, True) == (10, 20, 200), "round_dim rounds the height up"
    assert model.conve_image_shape(8, 2) == (2, 4, 8) and model.conve_image_shape(18, 2) == (3, 6, 18)
    with pytest.raises(Exception, match="incompatible with aspect ratio"):
        model.conve_image_shape(190)
    assert engine.conve_gate(10, 20, 3, 0) and engine.conve_gate(10, 20, 1, 2)
    assert not engine.conve_gate(20, 40, 1, 2) and not engine.conve_gate(10, 20, 6, 0)
    for opt in ("fused_dist_loss", "fused_f32_loss"):
        with pytest.raises(ValueError, match=opt):
            model.create("conve", 9, 3, 8, **{opt: True})
    m = model.create("conve", 9, 3, 8)
    assert list(m.state_dict()) == [
        "_entity_embedder._embeddings.weight", "_relation_embedder._embeddings.weight", "_scorer.convolution.weight",
        "_scorer.convolution.bias", "_scorer.bn1.running_mean", "_scorer.bn1.running_var",
        "_scorer.bn1.num_batches_tracked", "_scorer.bn2.running_mean", "_scorer.bn2.running_var",
        "_scorer.bn2.num_batches_tracked", "_scorer.projection.weight", "_scorer.projection.bias"]
    assert tuple(m.get_s_embedder().weight.shape) == (9, 9) and tuple(m.get_p_embedder().weight.shape) == (3, 9)
    assert tuple(m.get_scorer().projection.weight.shape) == (8, 32 * 2 * 2)
    assert "_scorer.convolution.bias" not in model.create("conve", 9, 3, 8, convolution_bias=False).state_dict()
    z = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(9, 9), torch.zeros(1, dtype=torch.int32)))
    for call in (lambda: m.score_neg(z, z, z, 2, z.view(2, 1)), lambda: m.score_neg_shared(z, z, z, 2, z),
                 lambda: m.score_neg_blocks(z, z, z, None, z.view(2, 1))):
        with pytest.raises(ValueError, match="negative-sampling blocks"):
            call()
    with pytest.raises(ValueError, match="ConvE can only score objects"):
        m.score_spo(z, z, z)
    with pytest.raises(ValueError, match="ConvE can only score objects"):
        m.score_spo(z, z, z, "s")
    for call, combine in ((lambda: m.score_po(z, z), "_po"), (lambda: m.score_sp_po(z, z, z), "_po"),
                          (lambda: m.score_so(z, z), "s_o"),
                          (lambda: m.get_scorer().score_emb(torch.zeros(2, 9), torch.zeros(2, 9), torch.zeros(2, 9), "_po"),
                           "_po")):
        with pytest.raises(Exception, match="Combine {} not supported in ConvE's score function".format(combine)):
            call()
    # CPU parameters: the torch route, in both modes
    m.eval()
    with torch.no_grad():
        assert not m.kernel_route()
        assert tuple(m.score_sp(z, z).shape) == (2, 9) and tuple(m.score_spo(z, z, z, "o").shape) == (2,)
        assert tuple(m.score_sp(z, z, torch.tensor([1, 4, 5])).shape) == (2, 3)
    assert m.routes == {"kernel": 0, "torch": 3}
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.conve_queries(m.get_scorer().kernel_net(), m.get_s_embedder().weight, m.get_p_embedder().weight, z, z)
