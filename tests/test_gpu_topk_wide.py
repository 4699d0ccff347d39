"""kge_topk for 128 < k <= 1024 (topk_wide.hip: pending keys in LDS, a wave merges them by rank into the list in the
workspace, a bitonic fold merges the groups' lists) against tests/_topk_ref.py fed with the matrix the store entries
write -- ids equal, values equal bit for bit, as test_gpu_topk.py demands of the narrow kernels, whose helpers it uses."""
import numpy as np
import pytest
import torch

import _topk_ref as ref
import test_gpu_topk as base
from test_gpu_topk import DEV, eng  # noqa: F401  (`eng`: the engine fixture)

pytestmark = pytest.mark.gpu
N, M = 130, 5003


@pytest.fixture(scope="module")
def complex_case(eng):
    """ComplEx on float32 tables, d = 32, 130 queries, and their score matrix over 5003 columns, made once: every shape
    below is a corner of it (a score's bits do not depend on the launch that stored it: the canonical chain)."""
    T = base._tables(eng, "complex", M, 4, 32, torch.float32, seed=21)
    a, p = base._queries(np.random.default_rng(21), N, M, 4)
    return T, a, p, base._scores(eng, T, "complex", torch.float32, "sp_", a, p, 0, M)


@pytest.mark.parametrize("col_tiles", [1, 3, None])  # 1, 3: a group sees fewer than k columns, its lists stay short
@pytest.mark.parametrize("k", [129, 200, 256, 1000, 1024])
def test_bounds_of_k(eng, kge_switch, complex_case, k, col_tiles):
    T, a, p, sc = complex_case
    if col_tiles is not None:
        kge_switch.set("TOPK_COL_TILES", col_tiles)
    for n in (1, 65, N):          # 65, 130: a ragged last row block
        for m in (k - 1, 1000, M):  # k - 1: every row is padded; 5003: a ragged last tile
            base._check(eng.topk(T, "sp_", a[:n], p[:n], k, col_end=m), ref.topk_ref(sc[:n, :m], k), (n, m))


@pytest.mark.parametrize("col_tiles", [2, None])
@pytest.mark.parametrize("model", ["distmult", "transe"])
def test_equal_scores_order_by_ascending_id(eng, kge_switch, model, col_tiles):
    E, k = 3000, 256
    T = base._tables(eng, model, E, 3, 7, torch.float32, seed=2, integer=True)
    a, p = base._queries(np.random.default_rng(2), 65, E, 3)
    sc = base._scores(eng, T, model, torch.float32, "sp_", a, p, 0, E)
    want = ref.topk_ref(sc, k + 1)
    assert len(np.unique(sc)) < 200 and np.any(want[0][:, k - 1] == want[0][:, k])  # equal scores straddle position k
    if col_tiles is not None:
        kge_switch.set("TOPK_COL_TILES", col_tiles)
    base._check(eng.topk(T, "sp_", a, p, k), ref.topk_ref(sc, k))


@pytest.mark.parametrize("col_tiles", [2, None])
def test_filters_keep_slice_and_non_finite_scores(eng, kge_switch, col_tiles):
    """base._filter_case: row 0 unfiltered, row 1 emptied, row 2 left with five columns (< k), row 3's keep id listed;
    two table rows carry an inf (their columns score +-inf), one a NaN (its column scores NaN against every query)."""
    E, n, k, lo, m = 1500, 70, 256, 37, 1400
    T = base._tables(eng, "complex", E, 4, 32, torch.float32, seed=4)
    for row, col, x in ((41, 3, "inf"), (700, 5, "nan"), (1436, 17, "inf")):
        T.ent[row, col] = float(x)
    rng = np.random.default_rng(4)
    a, p = base._queries(rng, n, E, 4)
    keep = rng.integers(lo, lo + m, n)
    sets = base._filter_case(rng, n, E, lo, m, keep)
    sc = base._scores(eng, T, "complex", torch.float32, "sp_", a, p, lo, lo + m)
    assert np.isnan(sc).any() and np.isneginf(sc).any()
    if col_tiles is not None:
        kge_switch.set("TOPK_COL_TILES", col_tiles)
    for kp in (None, keep):
        want = ref.topk_ref(sc, k, sets, kp, col_begin=lo)
        if kp is None:
            assert np.all(want[1][1] == -1) and np.sum(want[1][2] >= 0) == 5
        got = eng.topk(T, "sp_", a, p, k, base._dev_filters(sets), None if kp is None else torch.from_numpy(kp).to(DEV),
                       lo, lo + m)
        base._check(got, want, kp is None)


@pytest.mark.parametrize("model,l_norm,dtype", [("distmult", 1.0, torch.float32), ("transe", 1.0, torch.float32),
                                                ("transe", 2.0, torch.float32), ("rotate", 1.0, torch.float32),
                                                ("complex", 1.0, torch.bfloat16)])
def test_scorers_and_dtypes(eng, model, l_norm, dtype):
    E, k = 2000, 256  # d = 24: the scalar-load path
    T = base._tables(eng, model, E, 5, 24, dtype, seed=24, l_norm=l_norm)
    a, p = base._queries(np.random.default_rng(24), 65, E, 5)
    for direction in ("sp_", "_po"):
        want = ref.topk_ref(base._scores(eng, T, model, dtype, direction, a, p, 0, E), k)
        base._check(eng.topk(T, direction, a, p, k), want, direction)


@pytest.mark.parametrize("k", [1, 10, 128])
def test_the_two_kernel_pairs_agree(eng, kge_switch, complex_case, k):
    T, a, p, sc = complex_case
    kge_switch.set("TOPK_WIDE", 2)
    narrow = eng.topk(T, "sp_", a, p, k)
    kge_switch.set("TOPK_WIDE", 1)
    wide = eng.topk(T, "sp_", a, p, k)
    assert torch.equal(narrow[1], wide[1]) and torch.equal(narrow[0].view(torch.int32), wide[0].view(torch.int32))
    base._check(wide, ref.topk_ref(sc, k))
