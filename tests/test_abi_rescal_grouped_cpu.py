"""The relation-grouped RESCAL entries at the C ABI without a device: exported and bound, the gate (answers before any
launch: the table pointers below are never dereferenced), the workspace rule, and the front end's `grouped` option."""
import ctypes

import pytest
import torch

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -5
GROUPED = 1 << 17  # KGE_FLAG_RESCAL_GROUPED
NAMES = ("kge_rescal_grouped_workspace_bytes", "kge_rescal_group", "kge_rescal_queries_grouped",
         "kge_score_neg_bwd_accum_grouped")


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def _tables(dtype=0, scorer=5, dim=8, rel_dim=64, flags=GROUPED):
    from kge_amd._lib import KgeTables
    return KgeTables(4096, 8192, dtype, scorer, 10, 3, dim, rel_dim, dim, rel_dim, 1.0, flags)


def _calls(lib, t, n, ws, ws_bytes, slot=2):
    from kge_amd._lib import KgeIndex
    ix, tp = KgeIndex(4096, 1, 0, 1), ctypes.byref(t)
    return (lib.kge_rescal_group(tp, ix, n, ws, ws_bytes, None),
            lib.kge_rescal_queries_grouped(tp, 1, ix, ix, n, 4096, t.dim, ws, ws_bytes, None),
            lib.kge_score_neg_bwd_accum_grouped(tp, ix, ix, ix, n, slot, 4096, 1, 2, 2, 4096, 2, None, 0, 4096, t.dim, 4096,
                                                t.rel_dim, ws, ws_bytes, None))


def test_symbols_are_exported_and_bound(lib):
    from kge_amd import _lib, engine
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert _lib.FLAG_RESCAL_GROUPED == GROUPED and engine.RESCAL_GROUPED_MAX_N == 65536
    for fn in ("rescal_group", "rescal_queries", "score_neg_bwd_accum_grouped"):
        assert callable(getattr(engine, fn))


@pytest.mark.parametrize("bad", [dict(scorer=0, rel_dim=8), dict(scorer=1, rel_dim=8), dict(scorer=2, rel_dim=8),
                                 dict(scorer=3, rel_dim=4), dict(scorer=4, rel_dim=16), dict(dtype=1),
                                 dict(dim=257, rel_dim=257 * 257), dict(flags=0)], ids=str)
def test_the_gate_declines_before_any_launch(lib, bad):
    t = _tables(**bad)
    assert lib.kge_rescal_grouped_workspace_bytes(ctypes.byref(t), 5) == 0
    assert _calls(lib, t, 5, 4096, 1 << 30) == (UNSUPPORTED,) * 3


def test_workspace_rule_and_arguments(lib):
    t = _tables()
    need = lib.kge_rescal_grouped_workspace_bytes(ctypes.byref(t), 5)
    a16 = lambda b: (b + 15) & ~15
    assert need >= 3 * a16(20) + a16(24) + 16 + 2 * 5 * 8 * 4 and need % 16 == 0
    for ws, nbytes in ((None, 0), (None, need), (4096, need - 4)):
        assert _calls(lib, t, 5, ws, nbytes) == (WORKSPACE,) * 3
    assert _calls(lib, t, 0, None, 0) == (0, 0, 0)  # n == 0: nothing to do, nothing touched
    assert _calls(lib, t, 5, 4096, need, slot=1)[2] == INVALID  # the ungrouped entry's rule for the relation slot
    assert lib.kge_rescal_grouped_workspace_bytes(ctypes.byref(t), 65537) == 0
    assert _calls(lib, t, 65537, 4096, 1 << 40) == (UNSUPPORTED,) * 3


def test_create_declines_what_the_grouped_route_cannot_serve():
    from kge_amd import model
    m = model.create("rescal", 40, 5, 6, grouped=True)
    assert m.grouped and model.create("relational_tucker3", 40, 5, 6, rel_base_dim=3, grouped=True).grouped
    assert not model.create("rescal", 40, 5, 6).grouped
    with pytest.raises(ValueError, match="grouped.*fused_dropout"):
        model.create("rescal", 40, 5, 6, grouped=True, fused_dropout=True)
    with pytest.raises(ValueError, match="grouped"):
        model.create("distmult", 40, 5, 6, grouped=True)
    with pytest.raises(ValueError, match="grouped.*touched_rows"):
        m.set_touched_rows((torch.zeros(40, 6), torch.zeros(2, dtype=torch.int32)))
    i = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="grouped.*shared"):
        m.score_neg_shared(i, i, i, 2, torch.arange(4))
