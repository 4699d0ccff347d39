"""The training entries of ConvE (kge_conve_train_*) without a GPU: the symbols, the gate reached before any launch, n == 0,
and the fused_train option of the model."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    return _lib.lib()


def _net(h=4, w=8, filter_size=3, padding=0):
    from kge_amd import _lib
    F = max(32 * (2 * h - filter_size + 2 * padding + 1) * (w - filter_size + 2 * padding + 1), 1)
    return _lib.KgeConveNet(h, w, filter_size, padding, 1, 0, 16, 16, None, None, 16, F, 16, None, None, 1e-5, 1e-5)


def _calls(lib, c, n, p=(0.2, 0.3), ws=16, ws_bytes=1 << 40, tr=True):
    from kge_amd import _lib
    t = ctypes.byref(_lib.KgeConveTrain(p[0], p[1], 7, 1)) if tr else None
    d, F = c.h * c.w, c.proj_ld
    b = None if n == 0 else 16
    return (lib.kge_conve_train_fwd(ctypes.byref(c), t, b, d + 1, b, d + 1, n, b, d, b, b, b, b, b, ws, ws_bytes, None),
            lib.kge_conve_train_bwd(ctypes.byref(c), t, b, d + 1, b, d + 1, n, b, d, b, b, b, b, b, b, d + 1, b, d + 1, b,
                                    b, b, F, b, ws, ws_bytes, None))


def test_symbols_and_gate_before_any_launch(lib):
    from kge_amd import _lib
    for name in ("kge_conve_train_workspace_bytes", "kge_conve_train_fwd", "kge_conve_train_bwd"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert ctypes.sizeof(_lib.KgeConveTrain) == 24
    c = _net()
    need = lib.kge_conve_train_workspace_bytes(ctypes.byref(c), 5)
    assert need >= 32 * 5 * 32 * 4, "at least the channel partials"
    for bad, n in ((c, 1), (_net(filter_size=6), 5), (_net(padding=3), 5)):
        assert _calls(lib, bad, n) == (UNSUPPORTED, UNSUPPORTED)
        assert lib.kge_conve_train_workspace_bytes(ctypes.byref(bad), n) == 0
    for p in ((1.0, 0.0), (0.0, -0.1), (float("nan"), 0.0)):
        assert _calls(lib, c, 5, p=p) == (UNSUPPORTED, UNSUPPORTED), p
    assert _calls(lib, c, 5, ws=None) == (WORKSPACE, WORKSPACE)
    assert _calls(lib, c, 5, ws_bytes=need - 1) == (WORKSPACE, WORKSPACE)
    assert _calls(lib, c, 5, tr=False) == (INVALID, INVALID) and _calls(lib, c, -1) == (INVALID, INVALID)
    assert _calls(lib, _net(padding=3), 5, tr=False) == (INVALID, INVALID), "an argument error in front of the shape"
    assert _calls(lib, c, 0, ws=None, ws_bytes=0) == (OK, OK), "n == 0 launches nothing"


def test_the_option_builds_and_is_off_by_default():
    from kge_amd import engine, model
    m = model.create("conve", 40, 5, 32, fused_train=True)
    assert m.routes == {"kernel": 0, "torch": 0, "train": 0} and m.get_scorer().fused_train
    assert model.create("conve", 40, 5, 32).routes == {"kernel": 0, "torch": 0}
    assert engine.conve_train_supported(4, 8, 3, 0, 2) and not engine.conve_train_supported(4, 8, 3, 0, 1)
    assert not engine.conve_train_supported(4, 8, 6, 0, 8)
