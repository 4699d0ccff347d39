"""tests/_touched_ref.py -- the numpy restatement of kge_touched_mark / kge_adagrad_step_touched that the GPU tests
compare bits with -- checked on the CPU, and what of the new entry points answers without a device.

The yardstick of the whole feature: a dense Adagrad step with weight_decay == 0 leaves a row whose
gradient is zero bit for bit as it was (sum + 0 * 0 = sum; p + (minus_clr * 0) / (sqrt(sum) + eps) = p, signed zeros
included), so the step over the marked rows must equal the dense step over every row -- in parameter AND accumulator,
for gradients that are zero outside the marked rows."""
import ctypes
import os

import numpy as np
import pytest

import _optim_ref as orf
import _touched_ref as tr

from conftest import ROOT

ES = [1, 31, 32, 33, 2047, 2048, 2049, 4100]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


@pytest.mark.parametrize("E", ES)
def test_bitmap_bytes_and_mark_are_packbits_set_logic(E):
    rng = np.random.default_rng(E)
    assert tr.bitmap_bytes(E) % 16 == 0 and 0 <= tr.bitmap_bytes(E) - 4 * ((E + 31) // 32) < 16
    assert tr.bitmap_bytes(0) == 0
    for ids in (np.zeros(0, np.int64), np.arange(E), np.array([0]), np.array([E - 1]),
                np.array([x for x in (32 * ((E - 1) // 32), 32 * ((E - 1) // 32) + 31) if x < E]),
                rng.integers(0, E, 3 * E + 5), np.array([-1, E, E + 31, 2 ** 40, -2 ** 40, E // 2])):
        got = tr.mark(ids, E)
        member = np.zeros(got.size * 32, dtype=np.uint8)
        ok = ids[(ids >= 0) & (ids < E)]
        member[ok] = 1
        want = np.packbits(member, bitorder="little").view(np.uint32)
        assert np.array_equal(got, want)
        assert tr.marked_rows(got, E) == sorted(set(int(x) for x in ok))
    # marks accumulate
    a = tr.mark([0, E - 1], E)
    assert np.array_equal(tr.mark([E // 2], E, a), tr.mark([0, E - 1, E // 2], E))


@pytest.mark.parametrize("E,dim", [(1, 1), (33, 5), (70, 8), (2049, 4), (300, 130)])
def test_step_over_the_marked_rows_is_the_dense_step(E, dim):
    rng = np.random.default_rng(E * 1000 + dim)
    p = rng.standard_normal((E, dim)).astype(np.float32)
    p[rng.random((E, dim)) < 0.05] = -0.0      # signed zeros must survive on untouched rows
    p[rng.random((E, dim)) < 0.02] = 1e-42     # ... and denormals
    s = (rng.random((E, dim)) * 3).astype(np.float32)
    s[rng.random((E, dim)) < 0.1] = 0.0         # a fresh accumulator: sqrt(0) + eps
    rows = np.unique(rng.integers(0, E, max(1, E // 3)))
    g = np.zeros((E, dim), dtype=np.float32)
    g[rows] = rng.standard_normal((rows.size, dim)).astype(np.float32)
    zero_row = rows[0]
    g[zero_row] = 0.0                           # a marked row whose gradient is all zero
    g[rows[-1], 0] = -0.0
    bitmap = tr.mark(rows, E)
    # (eps > 0: with eps == 0 a fresh accumulator makes the DENSE step 0 / 0 on a row without a gradient)
    for minus_clr, eps in ((-0.05, 1e-10), (-1.0, 1e-30), (-0.3, 1e-3)):
        p1, g1, s1, b1, c1 = tr.step_touched(p, g, s, bitmap, minus_clr, eps, copy=np.full((E, dim), 0xBEEF, np.uint16))
        p2, s2 = tr.dense_adagrad(p, g, s, minus_clr, eps)
        nan = np.isnan(p2)
        assert np.array_equal(_bits(p1)[~nan], _bits(p2)[~nan]) and np.array_equal(np.isnan(p1), nan)
        assert np.array_equal(_bits(s1), _bits(s2))
        # ... and the restatement the dense kernels are already held to (tests/test_gpu_optim_exact.py)
        p3, s3 = orf.adagrad(p, g, s, minus_clr, 0.0, eps)
        assert np.array_equal(_bits(p2.reshape(-1))[~nan.reshape(-1)], _bits(p3)[~nan.reshape(-1)])
        assert np.array_equal(_bits(s2.reshape(-1)), _bits(s3))
        assert not g1.any() and not _bits(g1).any() and not b1.any()
        touched = np.zeros(E, bool)
        touched[rows] = True
        assert np.array_equal(c1[touched], orf.bf16_rne_bits(p1[touched])) and (c1[~touched] == 0xBEEF).all()
        assert np.array_equal(_bits(p1[~touched]), _bits(p[~touched]))


def test_unmarked_rows_are_not_looked_at():
    """A gradient OUTSIDE the marked rows stays where it is and moves nothing (the kernel's contract; the optimizer's
    invariant -- zero outside the marked rows -- is the backward's to keep)."""
    p = np.ones((4, 3), np.float32)
    g = np.full((4, 3), 2.0, np.float32)
    s = np.zeros((4, 3), np.float32)
    p1, g1, s1, b1, _ = tr.step_touched(p, g, s, tr.mark([2], 4), -0.5, 1e-10)
    assert (p1[[0, 1, 3]] == 1).all() and (g1[[0, 1, 3]] == 2).all() and (s1[[0, 1, 3]] == 0).all()
    assert (g1[2] == 0).all() and (s1[2] == 4).all() and not b1.any()


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def test_entry_points_answer_without_a_device(lib):
    from kge_amd._lib import KgeIndex, PROTOTYPES
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    for name in ("kge_touched_bitmap_bytes", "kge_touched_mark", "kge_adagrad_step_touched"):
        assert name in PROTOTYPES and f" {name}(" in header
    for E in [0] + ES + [4594485]:
        assert lib.kge_touched_bitmap_bytes(E) == tr.bitmap_bytes(E)
    P = ctypes.c_void_p(16)
    good, null = KgeIndex(P, 1, 0, 3), KgeIndex(None, 1, 0, 1)
    assert lib.kge_touched_mark(null, 0, 1, 1, 10, None, None) == 0        # nothing to mark: no launch
    assert lib.kge_touched_mark(good, 5, 0, 0, 10, None, None) == 0
    assert lib.kge_touched_mark(null, 5, 1, 1, 10, P, None) == -1          # no ids
    assert lib.kge_touched_mark(good, 5, 1, 1, 10, None, None) == -1       # no bitmap
    assert lib.kge_touched_mark(good, 5, 4, 3, 10, P, None) == -1          # ld < k
    assert lib.kge_touched_mark(good, -1, 1, 1, 10, P, None) == -1
    assert lib.kge_touched_mark(KgeIndex(P, 7, 0, 1), 5, 1, 1, 10, P, None) == -1   # neither int32 nor int64
    assert lib.kge_touched_mark(KgeIndex(P, 1, 0, 0), 5, 1, 1, 10, P, None) == -1   # stride < 1
    step = lambda p=P, g=P, s=P, b=P, E=10, d=8, ld=8, c=None, cld=0: lib.kge_adagrad_step_touched(
        p, ld, g, ld, s, ld, b, E, d, -0.1, 1e-10, c, cld, None)
    assert step(E=0) == 0                                                   # an empty table: no launch
    assert step(p=None) == -1 and step(g=None) == -1 and step(s=None) == -1 and step(b=None) == -1
    assert step(ld=7) == -1 and step(c=P, cld=7) == -1 and step(E=-1) == -1 and step(d=-1) == -1


def test_the_option_is_off_by_default_and_adagrad_refuses_what_the_row_step_cannot_do():
    import torch
    import yaml
    from kge_amd.optim import Adagrad
    cfg = yaml.safe_load(open(os.path.join(ROOT, "kge_amd", "libkge_plugin", "hip_negative_sampling.yaml")))
    assert cfg["hip_negative_sampling"]["touched_rows"] is False
    w = torch.nn.Parameter(torch.zeros(4, 3))
    opt = Adagrad([w], lr=0.1)
    assert opt.touched_rows(w) is None and opt.stepped_params() == []
    with pytest.raises(ValueError):
        opt.enable_touched_rows(w)                       # not on a GPU
    with pytest.raises(ValueError):
        opt.enable_touched_rows(torch.nn.Parameter(torch.zeros(4, 3)))  # not this optimizer's
    w.grad = torch.ones(4, 3)
    opt.step()                                           # (torch's own update: a CPU parameter)
    assert [q is w for q in opt.stepped_params()] == [True]
