"""kge_topk (filtered top-k prediction inside the exact scoring kernel) against the route it replaces: the score matrix
of kge_score_sp / kge_score_po on the same tables (KGE_FLAG_EXACT for bf16 ComplEx / DistMult), fed to the numpy
restatement tests/_topk_ref.py (canonicalise, drop the filtered columns, stable sort on (-value, id), pad).  Everything
is exact: ids equal, values equal bit for bit -- the kernel sees the very bits the score entries store, and the ordering
rule decides every element."""
import ctypes

import numpy as np
import pytest
import torch

import _topk_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DOT = ("complex", "distmult")


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _tables(eng, model, E, R, d, dtype, seed, l_norm=1.0, integer=False):
    g = torch.Generator().manual_seed(seed)
    dr = d // 2 if model == "rotate" else d
    if integer:  # |x| <= 2: exact in bf16 and in every sum -- many equal scores
        ent = torch.randint(-2, 3, (E, d), generator=g).float()
        rel = torch.randint(-2, 3, (R, dr), generator=g).float()
    else:
        ent = torch.randn(E, d, generator=g) * 0.5
        rel = torch.randn(R, dr, generator=g) * 0.5
    return eng.Tables(model, ent.to(dtype).to(DEV), rel.to(dtype).to(DEV), l_norm)


def _ref_flags(model, dtype):
    from kge_amd import _lib
    return _lib.FLAG_EXACT if (dtype == torch.bfloat16 and model in DOT) else 0


def _scores(eng, T, model, dtype, direction, a, p, lo, hi):
    """The reference's score matrix: the existing store entries on the same tables."""
    tg = None if (lo == 0 and hi == T.num_ent) else range(lo, hi)
    fl = _ref_flags(model, dtype)
    sc = eng.score_sp(T, a, p, tg, flags=fl, padded=False) if direction == "sp_" else \
        eng.score_po(T, p, a, tg, flags=fl, padded=False)
    return sc.cpu().numpy()


def _queries(rng, n, E, R):
    return (torch.from_numpy(rng.integers(0, E, n)).to(DEV), torch.from_numpy(rng.integers(0, R, n)).to(DEV))


def _check(got, want, what=""):
    val, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert val.dtype == np.float32 and idx.dtype == np.int64 and val.shape == want[0].shape
    assert np.array_equal(idx, want[1]), what
    assert np.array_equal(val.view(np.uint32), want[0].view(np.uint32)), what


def _dev_filters(filters):
    return [tuple(torch.from_numpy(np.asarray(x, dtype=np.int64)).to(DEV) for x in f) for f in filters]


# ---- scorers, dtypes, directions, dims -------------------------------------------------------------------------------
MODELS = [("complex", 1.0), ("distmult", 1.0), ("transe", 1.0), ("transe", 2.0), ("rotate", 1.0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("model,l_norm", MODELS)
@pytest.mark.parametrize("d", [7, 64, 128])
def test_scorers_dtypes_directions(eng, model, l_norm, d, dtype):
    if d % 2 and model in ("complex", "rotate"):
        d = 6  # (complex coordinates: an even dimension; still the scalar-load path)
    E, R, n, k = 1000, 5, 65, 10
    T = _tables(eng, model, E, R, d, dtype, seed=d, l_norm=l_norm)
    rng = np.random.default_rng(d)
    a, p = _queries(rng, n, E, R)
    for direction in ("sp_", "_po"):
        want = ref.topk_ref(_scores(eng, T, model, dtype, direction, a, p, 0, E), k)
        _check(eng.topk(T, direction, a, p, k), want, (model, direction))


# ---- n, m, col_begin, k ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_case(eng):
    """One DistMult / one TransE table pair and 130 queries, made once: every shape below is a slice of them."""
    out = {}
    for model in ("distmult", "transe"):
        T = _tables(eng, model, 5003 + 37, 4, 64, torch.float32, seed=11)
        rng = np.random.default_rng(5)
        a, p = _queries(rng, 130, T.num_ent, 4)
        out[model] = (T, a, p)
    return out


@pytest.mark.parametrize("model", ["distmult", "transe"])
@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000, 5003])
def test_rows_columns_slices(eng, shape_case, model, n, m):
    T, a, p = shape_case[model]
    a, p = a[:n], p[:n]
    for lo in (0, 37):
        sc = _scores(eng, T, model, torch.float32, "sp_", a, p, lo, lo + m)
        for k in (1, 10, 64, 128):  # (k > m for the small slices: padding)
            _check(eng.topk(T, "sp_", a, p, k, col_begin=lo, col_end=lo + m), ref.topk_ref(sc, k, col_begin=lo), (lo, k))


@pytest.mark.parametrize("model", ["distmult", "transe"])
@pytest.mark.parametrize("m", [1000, 5003])
@pytest.mark.parametrize("col_tiles", [1, 3, None])
def test_result_does_not_depend_on_the_column_groups(eng, kge_switch, shape_case, model, m, col_tiles):
    T, a, p = shape_case[model]
    if col_tiles is not None:
        kge_switch.set("TOPK_COL_TILES", col_tiles)
    sc = _scores(eng, T, model, torch.float32, "_po", a, p, 0, m)
    for k in (10, 128):
        _check(eng.topk(T, "_po", a, p, k, col_end=m), ref.topk_ref(sc, k), (col_tiles, k))


# ---- forced ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("model", ["distmult", "transe"])
@pytest.mark.parametrize("col_tiles", [1, None])
def test_equal_scores_order_by_ascending_id(eng, kge_switch, model, dtype, col_tiles):
    E, R, d, n, k = 1000, 3, 7, 65, 10
    T = _tables(eng, model, E, R, d, dtype, seed=2, integer=True)
    rng = np.random.default_rng(2)
    a, p = _queries(rng, n, E, R)
    sc = _scores(eng, T, model, dtype, "sp_", a, p, 0, E)
    want = ref.topk_ref(sc, k + 1)
    assert len(np.unique(sc)) < 200  # far fewer distinct values than columns
    assert np.any(want[0][:, k - 1] == want[0][:, k]), "no row has equal scores straddling position k"
    if col_tiles is not None:
        kge_switch.set("TOPK_COL_TILES", col_tiles)
    _check(eng.topk(T, "sp_", a, p, k), ref.topk_ref(sc, k))
    _check(eng.topk(T, "sp_", a, p, 128), ref.topk_ref(sc, 128))


# ---- filters ---------------------------------------------------------------------------------------------------------
def _filter_case(rng, n, E, lo, m, keep):
    """Two overlapping sets as (begin, end, col).  Row 0: an empty range in both.  Row 1: every column of the slice (all
    padding).  Row 2: all but five columns (fewer than k left).  Row 3: its keep id listed.  Others: a few random
    columns, some outside the slice, some in both sets."""
    sets = []
    for f in range(2):
        begin, end, col = np.zeros(n, np.int64), np.zeros(n, np.int64), []
        for i in range(n):
            if i == 0:
                v = np.zeros(0, np.int64)
            elif i == 1:
                v = np.arange(lo, lo + m) if f == 0 else np.arange(lo, lo + m, 3)
            elif i == 2:
                v = np.setdiff1d(np.arange(lo, lo + m), lo + np.array([0, 1, m // 2, m - 2, m - 1]))[f::2]
            else:
                v = rng.choice(E, size=int(rng.integers(1, 40)), replace=False)
                if f == 1:
                    v = np.concatenate([v, sets[0][2][sets[0][0][i]:sets[0][1][i]][:3]])
            if i == 3:
                v = np.append(v, keep[i])
            begin[i] = len(col)
            col.extend(np.unique(v).tolist())
            end[i] = len(col)
        sets.append((begin, end, np.asarray(col, np.int64)))
    return sets


@pytest.mark.parametrize("model,dtype", [("complex", torch.bfloat16), ("distmult", torch.float32),
                                         ("transe", torch.float32), ("rotate", torch.bfloat16)])
@pytest.mark.parametrize("lo,m", [(0, 1000), (37, 900)])
def test_filters(eng, kge_switch, model, dtype, lo, m):
    E, R, d, n, k = 1000, 4, 64, 70, 10
    T = _tables(eng, model, E, R, d, dtype, seed=4)
    rng = np.random.default_rng(4)
    a, p = _queries(rng, n, E, R)
    keep = rng.integers(lo, lo + m, n)
    sets = _filter_case(rng, n, E, lo, m, keep)
    sc = _scores(eng, T, model, dtype, "sp_", a, p, lo, lo + m)
    keep_t = torch.from_numpy(keep).to(DEV)
    for use in (sets[:1], sets):
        for kp, kp_t in ((None, None), (keep, keep_t)):
            want = ref.topk_ref(sc, k, use, kp, col_begin=lo)
            if kp is None and len(use) == 2:
                assert np.all(want[1][1] == -1) and np.all(np.isneginf(want[0][1]))   # every column removed
                assert np.sum(want[1][2] >= 0) == 5                                     # fewer than k left
            for ct in (2, None):
                if ct is None:
                    kge_switch.unset("TOPK_COL_TILES")
                else:
                    kge_switch.set("TOPK_COL_TILES", ct)
                _check(eng.topk(T, "sp_", a, p, k, _dev_filters(use), kp_t, lo, lo + m), want, (len(use), kp is None, ct))
    # keep protects a listed column: row 1 (everything listed) keeps exactly its keep id
    want = ref.topk_ref(sc, k, sets, keep, col_begin=lo)
    assert want[1][1, 0] == keep[1] and np.all(want[1][1, 1:] == -1)


# ---- non-finite scores -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["distmult", "transe", "complex"])
def test_non_finite_scores_come_before_the_padding(eng, model):
    E, R, d, n = 100, 3, 64, 5
    T = _tables(eng, model, E, R, d, torch.float32, seed=6)
    T.ent[41, 3] = float("inf")  # column 41 scores +-inf or NaN against every row
    rng = np.random.default_rng(6)
    a, p = _queries(rng, n, E, R)
    a[a == 41] = 40
    sc = _scores(eng, T, model, torch.float32, "sp_", a, p, 0, E)
    assert not np.all(np.isfinite(sc[:, 41])) and np.all(np.isfinite(np.delete(sc, 41, axis=1)))
    k = 128  # > E: padding behind the real columns
    want = ref.topk_ref(sc, k)
    low = np.isnan(sc[:, 41]) | np.isneginf(sc[:, 41])
    if model != "complex":
        assert np.any(low)
    for i in np.nonzero(low)[0]:  # listed as -inf, last of the real columns, ahead of the padding
        assert want[1][i, E - 1] == 41 and np.isneginf(want[0][i, E - 1]) and want[1][i, E] == -1
    _check(eng.topk(T, "sp_", a, p, k), want)
    # the same with other -inf columns around it: -inf columns order by id
    T.ent[7, 5] = float("inf")
    T.ent[90, 1] = float("inf")
    sc = _scores(eng, T, model, torch.float32, "sp_", a, p, 0, E)
    _check(eng.topk(T, "sp_", a, p, k), ref.topk_ref(sc, k))


# ---- the C entry: workspace, pitch, side effects, status codes -------------------------------------------------------
def _raw_call(eng, T, a, p, k, m, val, idx, ld, ws, ws_bytes, flags=0, filters=(), lo=0, num_filters=None):
    from kge_amd import _lib
    keepalive = []
    ai, pi = eng._index(a, T.device, keepalive), eng._index(p, T.device, keepalive)
    K = len(filters) if num_filters is None else num_filters
    arr = ctypes.c_void_p * max(len(filters), 1)
    pb, pe, pc = (arr(*[f[j].data_ptr() for f in filters]) if filters else None for j in range(3))
    tc = T.c(flags)
    return _lib.lib().kge_topk(ctypes.byref(tc), _lib.SP_, ai, pi, a.numel(), lo, m, k, K, pb, pe, pc,
                               _lib.KgeIndex(None, _lib.I64, 0, 1), None if val is None else val.data_ptr(),
                               None if idx is None else idx.data_ptr(), ld, None if ws is None else ws.data_ptr(),
                               ws_bytes, eng._stream_handle(T.device))


def test_workspace_pitch_and_status_codes(eng):
    from kge_amd import _lib
    E, R, d, n, k, ld = 1000, 3, 64, 66, 10, 13
    T = _tables(eng, "distmult", E, R, d, torch.float32, seed=8)
    rng = np.random.default_rng(8)
    a, p = _queries(rng, n, E, R)
    sets = _dev_filters(_filter_case(rng, n, E, 0, E, rng.integers(0, E, n)))
    sc = _scores(eng, T, "distmult", torch.float32, "sp_", a, p, 0, E)
    want = ref.topk_ref(sc, k, [tuple(x.cpu().numpy() for x in f) for f in sets])
    tc = T.c(0)
    need = _lib.lib().kge_topk_workspace_bytes(ctypes.byref(tc), n, E, k, 2)
    assert need > 0
    # garbage in the workspace, canaries around and between the output rows
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    val = torch.full((n + 2, ld), 123.0, device=DEV)
    idx = torch.full((n + 2, ld), -77, dtype=torch.int64, device=DEV)
    for _ in range(2):  # the second call reuses the workspace as the first left it
        assert _raw_call(eng, T, a, p, k, E, val[1:], idx[1:], ld, ws, need, filters=sets) == 0
        torch.cuda.synchronize()
        _check((val[1:n + 1, :k], idx[1:n + 1, :k]), want)
        assert bool((val[0] == 123.0).all()) and bool((val[n + 1] == 123.0).all()) and bool((val[:, k:] == 123.0).all())
        assert bool((idx[0] == -77).all()) and bool((idx[n + 1] == -77).all()) and bool((idx[:, k:] == -77).all())
        assert bool((ws[need:] == 0xA5).all())
    ERR_ARG, ERR_UNSUP, ERR_WS = -1, _lib.KGE_ERR_UNSUPPORTED, -5
    assert _lib.lib().kge_status_string(ERR_WS) == b"workspace too small"
    assert _raw_call(eng, T, a, p, k, E, val, idx, ld, ws, need - 1, filters=sets) == ERR_WS
    assert _raw_call(eng, T, a, p, k, E, val, idx, ld, ws[1:], need, filters=sets) == ERR_WS   # misaligned
    assert _raw_call(eng, T, a, p, 0, E, val, idx, ld, ws, need) == ERR_ARG
    assert _raw_call(eng, T, a, p, _lib.TOPK_MAX + 1, E, val, idx, 200, ws, need) == ERR_ARG
    assert _raw_call(eng, T, a, p, k, E, val, idx, k - 1, ws, need) == ERR_ARG
    assert _raw_call(eng, T, a, p, k, E, None, idx, ld, ws, need) == ERR_ARG
    assert _raw_call(eng, T, a, p, k, E + 1, val, idx, ld, ws, need) == ERR_ARG
    assert _raw_call(eng, T, a, p, k, E, val, idx, ld, ws, need, num_filters=1) == ERR_ARG   # a missing filter pointer
    assert _raw_call(eng, T, a, p, k, E, val, idx, ld, ws, need, num_filters=3) == ERR_UNSUP
    assert _raw_call(eng, T, a, p, k, E, val, idx, ld, ws, need, flags=_lib.FLAG_SPLIT_QUERY) == ERR_UNSUP
    assert _raw_call(eng, T, a, p, k, E, val, idx, ld, ws, need, flags=_lib.FLAG_BF16_V3) == ERR_UNSUP
    # empty batch / empty slice
    assert _raw_call(eng, T, a[:0], p[:0], k, E, None, None, ld, None, 0) == 0
    val.fill_(5.0)
    idx.fill_(5)
    assert _raw_call(eng, T, a, p, k, 0, val, idx, ld, None, 0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isneginf(val[:n, :k]).all()) and bool((idx[:n, :k] == -1).all()) and bool((val[:, k:] == 5.0).all())


def test_ctypes_route_equals_the_extension_route(eng, monkeypatch):
    from kge_amd import _lib
    assert _lib.ext() is not None and eng._ext(), "kge_amd._C is part of the build"
    E, R, d, n, k = 1000, 3, 64, 65, 64
    T = _tables(eng, "rotate", E, R, d, torch.float32, seed=9)
    rng = np.random.default_rng(9)
    a, p = _queries(rng, n, E, R)
    keep = rng.integers(0, E, n)
    sets = _filter_case(rng, n, E, 0, E, keep)
    keep_t = torch.from_numpy(keep).to(DEV)
    via_ext = eng.topk(T, "_po", a, p, k, _dev_filters(sets), keep_t)
    monkeypatch.setattr(eng, "_EXT", False)
    via_ctypes = eng.topk(T, "_po", a, p, k, _dev_filters(sets), keep_t)
    assert torch.equal(via_ext[1], via_ctypes[1]) and torch.equal(via_ext[0].view(torch.int32), via_ctypes[0].view(torch.int32))
    _check(via_ctypes, ref.topk_ref(_scores(eng, T, "rotate", torch.float32, "_po", a, p, 0, E), k, sets, keep))
