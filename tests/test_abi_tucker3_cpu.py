"""The Tucker3 entries of the C ABI without a GPU: symbols and signatures, every rejection of the gate (with the *_bytes
queries returning 0), n == 0, and the front end's option refusals, route rule and cache on CPU tensors."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("kge_tucker3_project_bytes", "kge_tucker3_project", "kge_tucker3_project_bwd_workspace_bytes",
           "kge_tucker3_project_bwd")
OK, INVALID, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    return _lib.lib()


def _t(**kw):
    from kge_amd import _lib
    v = dict(base=16, proj=16, dtype=_lib.F32, reserved_=0, num_rel=5, dim=8, base_dim=5, base_ld=5, proj_ld=5)
    v.update(kw)
    return _lib.KgeTucker3(**v)


def _range(start=0):
    from kge_amd import _lib
    return _lib.KgeIndex(None, _lib.I64, start, 1)


def _project(lib, t, idx, n, out=16, ld=None):
    return lib.kge_tucker3_project(ctypes.byref(t), idx, n, out, t.dim * t.dim if ld is None else ld, None)


def _bwd(lib, t, idx, n, **kw):
    a = dict(g_out=16, g_ld=t.dim * t.dim, g_brows=16, g_brows_ld=t.base_dim, g_w=16, g_w_ld=t.base_dim, ws=16, ws_bytes=1 << 30)
    a.update(kw)
    return lib.kge_tucker3_project_bwd(ctypes.byref(t), idx, n, a["g_out"], a["g_ld"], a["g_brows"], a["g_brows_ld"],
                                       a["g_w"], a["g_w_ld"], a["ws"], a["ws_bytes"], None)


def test_symbols_signatures_and_constants(lib):
    from kge_amd import _lib, engine
    assert lib.kge_abi_version() == 1
    header = open(ROOT + "/include/kge_amd.h").read()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\(", header), name
    m = re.search(r"#define KGE_TUCKER3_MAX_BASE_DIM (\d+)", header)
    assert int(m.group(1)) == _lib.TUCKER3_MAX_BASE_DIM == engine.TUCKER3_MAX_BASE_DIM >= 512
    fields = re.search(r"typedef struct kge_tucker3 \{(.*?)\} kge_tucker3;", header, re.S).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names == [f[0] for f in _lib.KgeTucker3._fields_]
    assert ctypes.sizeof(_lib.KgeTucker3) == 64


def test_the_gate_rejects_before_any_launch(lib):
    from kge_amd import _lib
    n = 3
    for t in (_t(dtype=_lib.BF16), _t(dim=_lib.RESCAL_MAX_DIM + 1),
              _t(base_dim=_lib.TUCKER3_MAX_BASE_DIM + 1, base_ld=4096, proj_ld=4096)):
        assert _project(lib, t, _range(), n) == UNSUPPORTED
        assert _bwd(lib, t, _range(), n) == UNSUPPORTED
        assert lib.kge_tucker3_project_bytes(ctypes.byref(t), n) == 0
        assert lib.kge_tucker3_project_bwd_workspace_bytes(ctypes.byref(t), n) == 0
    for t in (_t(dtype=7), _t(dim=0), _t(base_dim=0), _t(num_rel=0), _t(base_ld=4), _t(proj_ld=4), _t(base=None),
              _t(proj=None)):
        assert _project(lib, t, _range(), n) == INVALID
        assert _bwd(lib, t, _range(), n) == INVALID
    t = _t()
    assert lib.kge_tucker3_project_bytes(None, n) == 0 and lib.kge_tucker3_project(None, _range(), n, 16, 64, None) == INVALID
    assert lib.kge_tucker3_project_bytes(ctypes.byref(t), n) == n * 64 * 4
    assert lib.kge_tucker3_project_bwd_workspace_bytes(ctypes.byref(t), n) >= n * 5 * 4
    assert lib.kge_tucker3_project_bytes(ctypes.byref(t), 0) == 0
    # every d_r >= 1 up to the cap passes the gate
    for dr in (1, 100, 512, _lib.TUCKER3_MAX_BASE_DIM):
        assert lib.kge_tucker3_project_bytes(ctypes.byref(_t(base_dim=dr, base_ld=dr, proj_ld=dr)), 1) == 256
    # malformed calls
    assert _project(lib, t, _range(), -1) == INVALID
    assert _project(lib, t, _range(), n, out=None) == INVALID
    assert _project(lib, t, _range(), n, ld=63) == INVALID
    assert _project(lib, t, _range(3), n) == INVALID, "a range past the table"
    assert _project(lib, t, _range(-1), n) == INVALID
    assert _project(lib, t, _lib.KgeIndex(16, _lib.I64, 1, 1), n) == INVALID, "start with an index vector"
    assert _project(lib, t, _lib.KgeIndex(16, 5, 0, 1), n) == INVALID, "index type"
    assert _project(lib, t, _lib.KgeIndex(16, _lib.I32, 0, 0), n) == INVALID, "stride"
    assert _bwd(lib, t, _range(), n, g_out=None) == INVALID
    assert _bwd(lib, t, _range(), n, g_ld=63) == INVALID
    assert _bwd(lib, t, _range(), n, g_brows_ld=4) == INVALID and _bwd(lib, t, _range(), n, g_w_ld=4) == INVALID
    assert _bwd(lib, t, _range(), n, ws=None) == -5 and _bwd(lib, t, _range(), n, ws_bytes=8) == -5  # KGE_ERR_WORKSPACE


def test_empty_calls_launch_nothing(lib):
    t = _t()
    assert _project(lib, t, _range(), 0, out=None) == OK
    assert _project(lib, t, _range(5), 0) == OK
    assert _bwd(lib, t, _range(), 0, g_out=None, ws=None, ws_bytes=0) == OK
    assert _bwd(lib, t, _range(), 3, g_brows=None, g_w=None, ws=None, ws_bytes=0) == OK, "no output wanted"


def test_model_refusals_routes_and_cache_on_cpu_tensors():
    from kge_amd import engine, model
    for opt in ("fused_dist_loss", "fused_f32_loss"):
        with pytest.raises(ValueError, match=opt):
            model.create("relational_tucker3", 9, 3, 4, rel_base_dim=2, **{opt: True})
    with pytest.raises(ValueError, match="dim"):
        model.create("relational_tucker3", 9, 3, 257, rel_base_dim=2, device="meta")
    with pytest.raises(ValueError, match="rel_base_dim"):
        model.create("relational_tucker3", 9, 3, 4, rel_base_dim=engine.TUCKER3_MAX_BASE_DIM + 1)
    with pytest.raises(ValueError, match="project"):
        model.create("relational_tucker3", 9, 3, 4, project="some")
    m = model.create("relational_tucker3", 9, 3, 4, rel_base_dim=2)
    assert [tuple(v.shape) for v in m.state_dict().values()] == [(9, 4), (3, 2), (16, 2)]
    assert type(m).__mro__[2].__name__ == "KgeModel" and m.get_scorer().name == "rescal"
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(9, 4), torch.zeros(1, dtype=torch.int32)))
    z = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="score_neg_shared"):
        m.score_neg_shared(z, z, z, 2, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.tucker3_project(torch.zeros(3, 2), torch.zeros(16, 2))
    # the route rule
    assert m.route(2) == "batch" and m.route(3) == "all" and m.route(2, "all") == "all" and m.route(5, "batch") == "batch"
    with torch.no_grad():
        assert m.route(2) == "all"
        m.projected_table_max_bytes = 3 * 16 * 4 - 1
        assert m.route(2) == "batch" and m.route(100) == "batch"
        m.projected_table_max_bytes = 1 << 30
    with pytest.raises(ValueError, match="project"):
        m.route(2, "none")
    # the cache (CPU tensors: torch's linear): one projection per parameter version, none kept with a gradient recorded
    B, W = m._bw()
    with torch.no_grad():
        a = m.projected_table()
        assert m.projected_table() is a and m.projections == 1
        assert torch.equal(a, torch.nn.functional.linear(B, W))
        rel, p2, rows = m._rel(torch.tensor([2, 0]), "batch")
        assert torch.equal(rel, a[[2, 0]]) and p2.tolist() == [0, 1] and rows
        assert m._rel(torch.tensor([2, 0]), "all")[2] is False
        W.mul_(2.0)  # an in-place update bumps the version
        b = m.projected_table()
        assert m.projections == 2 and b is not a and torch.equal(b, 2.0 * a)
        B.add_(1.0)
        assert m.projected_table() is not b and m.projections == 3
    live = m.projected_table()
    assert live.requires_grad and m.projections == 3 and m.projected_table() is not live
