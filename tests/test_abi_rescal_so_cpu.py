"""kge_score_so / kge_score_so_bwd_accum / kge_score_so_workspace_bytes for RESCAL tables, without a GPU: the opt-in gate
answers before anything is launched, and the workspace rule of the forward's K splits."""
import ctypes

import pytest
import torch

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -5
P = ctypes.c_void_p(16)  # never dereferenced on these paths
GROUPED = 1 << 17


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def _tables(dim=8, dtype=0, flags=GROUPED, R=3):
    from kge_amd._lib import KgeTables
    return KgeTables(P, P, dtype, 5, 10, R, dim, dim * dim, dim, dim * dim, 1.0, flags)


def _ix(ptr=P):
    from kge_amd._lib import KgeIndex
    return KgeIndex(ptr, 1, 0, 1)


def _fwd(lib, t, n=4, ws=None, wsb=0):
    return lib.kge_score_so(ctypes.byref(t), _ix(), _ix(), n, _ix(None), 3, P, 3, ws, wsb, None)


def _bwd(lib, t, n=4):
    return lib.kge_score_so_bwd_accum(ctypes.byref(t), _ix(), _ix(), n, _ix(None), 3, P, 3, None, 0, P, t.dim, P,
                                      t.rel_dim, None, 0, None)


@pytest.mark.parametrize("t", [_tables(flags=0), _tables(dtype=1), _tables(dim=257)], ids=["plain", "bf16", "dim257"])
def test_the_gate_declines_before_any_launch(lib, t):
    assert _fwd(lib, t) == UNSUPPORTED and _bwd(lib, t) == UNSUPPORTED
    assert lib.kge_score_so_workspace_bytes(ctypes.byref(t), 512, 237) == 0


def test_workspace_rule_and_empty_calls(lib):
    ws = lambda d, n=512, m=237: lib.kge_score_so_workspace_bytes(ctypes.byref(_tables(dim=d)), n, m)
    assert ws(32) == 0                                   # one K split: the scores are stored directly
    assert ws(33) == 2 * 512 * 237 * 4 and ws(128) == 4 * 512 * 237 * 4 and ws(256) == 8 * 512 * 237 * 4
    assert ws(128, n=0) == 0
    t = _tables(dim=64)
    assert _fwd(lib, t) == WORKSPACE and _fwd(lib, t, ws=P, wsb=2 * 4 * 3 * 4 - 1) == WORKSPACE
    assert _fwd(lib, t, n=0) == OK and _bwd(lib, t, n=0) == OK
    assert _fwd(lib, t, n=65535 * 64 + 1, ws=P, wsb=1 << 40) == UNSUPPORTED


def test_front_end():
    from kge_amd import engine
    assert engine.rescal_score_so_supported(torch.float32, 256, 512)
    assert not engine.rescal_score_so_supported(torch.float32, 257, 512)
    assert not engine.rescal_score_so_supported(torch.bfloat16, 64, 512)
    assert not engine.rescal_score_so_supported(torch.float32, 64, 65535 * 64 + 1)
    assert not engine.score_so_supported("rescal", torch.float32, 8, 512)
