"""The weighted-penalty entries (include/kge_amd.h, kge_amd/csrc/wpenalty.hip) without a GPU: they are declared, exported
and bound, kge_wpenalty_seg has the header's layout, and every refusal the header lists comes back before anything is
launched (the pointers below are made-up addresses: a call that got as far as a launch would not return these codes)."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
A = 0x7F0000001000  # a 16-byte aligned made-up address


@pytest.fixture(scope="module")
def L():
    from kge_amd import _lib
    _lib.build()
    return _lib


def test_entries_are_exported_and_the_record_has_the_headers_layout(L):
    lib = L.lib()
    for name in ("kge_penalty_count", "kge_adagrad_step_multi_wpenalty", "kge_adam_step_multi_wpenalty",
                 "kge_adagrad_step_touched_wpenalty", "kge_sparse_adam_step_touched_wpenalty"):
        assert name in L.PROTOTYPES and hasattr(lib, name)
    assert lib.kge_abi_version() == 1
    S = L.KgeWPenaltySeg
    assert ctypes.sizeof(S) == 48
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("kind", 0), ("p", 4), ("weight", 8), ("row_dim", 16), ("value", 24), ("counts", 32), ("m", 40)]
    assert lib.kge_status_string(UNSUPPORTED) == b"unsupported configuration"
    assert L.get_switch("PENALTY_COUNT_PLAIN") is None


def _ix(ptr=A, itype=None, start=0, stride=1):
    from kge_amd._lib import I64, KgeIndex
    return KgeIndex(ptr, I64 if itype is None else itype, start, stride)


def test_penalty_count_refusals_and_the_empty_block(L):
    f = L.lib().kge_penalty_count
    assert f(_ix(), 0, 1, 1, 10, A, None, None) == OK          # n * k == 0: no launch
    assert f(_ix(None), 4, 0, 0, 10, A, None, None) == OK
    assert f(_ix(), -1, 1, 1, 10, A, None, None) == INVALID
    assert f(_ix(), 4, -1, 1, 10, A, None, None) == INVALID
    assert f(_ix(), 4, 1, 1, -1, A, None, None) == INVALID
    assert f(_ix(), 4, 2, 1, 10, A, None, None) == INVALID      # ld < k
    assert f(_ix(), 4, 1, 1, 10, None, None, None) == INVALID   # no counts
    assert f(_ix(), 4, 1, 1, 10, A + 2, None, None) == INVALID  # misaligned counts
    assert f(_ix(None), 4, 1, 1, 10, A, None, None) == INVALID  # no ids
    assert f(_ix(itype=7), 4, 1, 1, 10, A, None, None) == INVALID
    assert f(_ix(stride=0), 4, 1, 1, 10, A, None, None) == INVALID
    assert f(_ix(start=1), 4, 1, 1, 10, A, None, None) == INVALID


def _pen(L, kind=1, p=2, weight=0.1, row_dim=8, value=A, counts=A, m=16):
    return L.KgeWPenaltySeg(kind, p, weight, row_dim, value, counts, m)


BAD_RECORDS = [
    (dict(kind=3), INVALID), (dict(kind=-1), INVALID), (dict(value=None), INVALID), (dict(value=A + 4), INVALID),
    (dict(counts=None), INVALID), (dict(counts=A + 2), INVALID), (dict(row_dim=0), INVALID), (dict(row_dim=7), INVALID),
    (dict(m=0), INVALID), (dict(m=-3), INVALID), (dict(kind=2, row_dim=4), INVALID),
    (dict(p=0), UNSUPPORTED), (dict(p=4), UNSUPPORTED), (dict(m=1 << 24), UNSUPPORTED),
]


@pytest.mark.parametrize("change,status", BAD_RECORDS)
def test_every_refusal_of_the_weighted_record_on_all_four_entries(L, change, status):
    lib = L.lib()
    pen = _pen(L, **change)
    count = 64 * 8
    ag = L.KgeAdagradSeg(A, A, A, None, count, -0.1, 0.0, 1e-10)
    assert lib.kge_adagrad_step_multi_wpenalty(ctypes.byref(ag), ctypes.byref(pen), 1, None) == status
    ad = L.KgeAdamSeg(A, A, A, A, None, A, count, 0.01, 0.9, 0.999, 0.0, 1e-8)
    assert lib.kge_adam_step_multi_wpenalty(ctypes.byref(ad), ctypes.byref(pen), 1, None) == status
    touched = INVALID if "row_dim" in change else status  # (row_dim != dim is refused first)
    assert lib.kge_adagrad_step_touched_wpenalty(A, 8, A, 8, A, 8, A, 64, 8, -0.1, 1e-10, None, 0, ctypes.byref(pen),
                                                 None) == touched
    assert lib.kge_sparse_adam_step_touched_wpenalty(A, 8, A, 8, A, 8, A, 8, A, 64, 8, A, 0.01, 0.9, 0.999, 1e-8, None,
                                                     0, ctypes.byref(pen), None) == touched


def test_the_existing_entries_lists_hold_for_the_new_ones(L):
    lib = L.lib()
    pen = _pen(L)
    ag = lambda **k: L.KgeAdagradSeg(*[k.get(n, d) for n, d in (("param", A), ("grad", A), ("sum", A), ("copy", None),
                                                                ("count", 512), ("clr", -0.1), ("wd", 0.0),
                                                                ("eps", 1e-10))])
    f = lib.kge_adagrad_step_multi_wpenalty
    assert f(ctypes.byref(ag()), ctypes.byref(pen), 9, None) == INVALID
    assert f(ctypes.byref(ag()), ctypes.byref(pen), -1, None) == INVALID
    assert f(None, ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ag()), None, 1, None) == INVALID              # the weighted entries need their records
    assert f(ctypes.byref(ag(param=None)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ag(grad=A + 4)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ag(copy=A + 2)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ag(count=-1)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ag(count=516)), ctypes.byref(pen), 1, None) == INVALID   # count % row_dim
    assert f(ctypes.byref(ag(count=0)), ctypes.byref(pen), 1, None) == OK          # nothing non-empty: no launch
    assert f(None, None, 0, None) == OK
    ad = lambda **k: L.KgeAdamSeg(*[k.get(n, d) for n, d in (("param", A), ("grad", A), ("m1", A), ("m2", A),
                                                             ("copy", None), ("clock", A), ("count", 512), ("lr", 0.01),
                                                             ("b1", 0.9), ("b2", 0.999), ("wd", 0.0), ("eps", 1e-8))])
    f = lib.kge_adam_step_multi_wpenalty
    assert f(ctypes.byref(ad(clock=None)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ad(clock=A + 4)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ad(b1=1.0)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ad(m2=None)), ctypes.byref(pen), 1, None) == INVALID
    assert f(ctypes.byref(ad()), None, 1, None) == INVALID
    assert f(ctypes.byref(ad(count=0)), ctypes.byref(pen), 1, None) == OK
    two = (L.KgeAdamSeg * 2)(ad(), ad())
    pens = (L.KgeWPenaltySeg * 2)(pen, pen)
    assert f(two, pens, 2, None) == INVALID                                        # one clock, two segments
    t = lib.kge_adagrad_step_touched_wpenalty
    assert t(A, 8, A, 8, A, 8, A, 64, 8, -0.1, 1e-10, None, 0, None, None) == INVALID      # no record
    assert t(A, 7, A, 8, A, 8, A, 64, 8, -0.1, 1e-10, None, 0, ctypes.byref(pen), None) == INVALID  # pitch < dim
    assert t(None, 8, A, 8, A, 8, A, 64, 8, -0.1, 1e-10, None, 0, ctypes.byref(pen), None) == INVALID
    assert t(A, 8, A, 8, A, 8, None, 64, 8, -0.1, 1e-10, None, 0, ctypes.byref(pen), None) == INVALID
    assert t(A, 8, A, 8, A, 8, A, -1, 8, -0.1, 1e-10, None, 0, ctypes.byref(pen), None) == INVALID
    assert t(A, 8, A, 8, A, 8, A, 0, 8, -0.1, 1e-10, None, 0, ctypes.byref(pen), None) == OK        # no rows: no launch
    s = lib.kge_sparse_adam_step_touched_wpenalty
    assert s(A, 8, A, 8, A, 8, A, 8, A, 64, 8, None, 0.01, 0.9, 0.999, 1e-8, None, 0, ctypes.byref(pen), None) == INVALID
    assert s(A, 8, A, 8, A, 8, A, 8, A, 64, 8, A, 0.01, 0.9, 1.0, 1e-8, None, 0, ctypes.byref(pen), None) == INVALID
    assert s(A, 8, A, 8, A, 8, A, 8, A, 64, 8, A, 0.01, 0.9, 0.999, 1e-8, None, 0, None, None) == INVALID
