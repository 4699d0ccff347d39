"""The bound of kge_topk without a GPU: KGE_TOPK_MAX = 1024 in the header and in the binding, engine.topk's argument check
at the bound (before any library call), and the composed fallback at a k of the new range."""
import os
import re

import numpy as np
import pytest
import torch

import _topk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bound_is_1024_in_header_and_binding():
    from kge_amd import _lib
    with open(os.path.join(ROOT, "include", "kge_amd.h")) as f:
        found = re.search(r"KGE_TOPK_MAX\s*=\s*(\d+)", f.read())
    assert _lib.TOPK_MAX == 1024 == int(found.group(1))


def test_engine_topk_accepts_1024_and_rejects_1025_before_any_library_call(monkeypatch):
    from kge_amd import _lib, engine

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(engine, "_ext", no_library)
    ix = torch.zeros(3, dtype=torch.int64)
    assert engine._topk_args("sp_", 1024, None)[1] == 1024
    with pytest.raises(ValueError, match="k must be"):
        engine.topk(None, "sp_", ix, ix, 1025)


def test_composed_fallback_serves_k_1000():
    from kge_amd.model import topk_composed
    rng = np.random.default_rng(7)
    s = rng.integers(-3, 4, size=(5, 1203)).astype(np.float32)  # many equal scores
    s[1, 17], s[2, 200], s[3, 5] = np.nan, -np.inf, -0.0
    filters = [(np.array([0, 3, 3, 3, 3]), np.array([3, 3, 3, 3, 503]), np.concatenate([[5, 64, 900], np.arange(500)]))]
    keep = np.array([64, 0, 0, 0, 7])
    val, idx = topk_composed(torch.from_numpy(s), 1000, [tuple(torch.from_numpy(x) for x in filters[0])],
                             torch.from_numpy(keep))
    want = ref.topk_ref(s, 1000, filters, keep)
    assert np.sum(want[1][4] >= 0) == 704  # fewer than k columns left: padded
    assert np.array_equal(idx.numpy(), want[1])
    assert np.array_equal(val.numpy().view(np.uint32), want[0].view(np.uint32))
