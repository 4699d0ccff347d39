"""Filtered top-k prediction without a GPU: the numpy restatement (tests/_topk_ref.py) against torch's sort, the 64-bit
key (monotone, round-trips), the merge of per-group lists against the one-group result, the torch composition behind
KgeModel.predict_o / predict_s on a CPU model, and engine.topk's argument checks (before any library call)."""
import numpy as np
import pytest
import torch

import _topk_ref as ref


def test_restatement_equals_a_descending_sort_on_tie_free_data():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((9, 301)).astype(np.float32)
    assert all(len(np.unique(r)) == len(r) for r in s)
    for k in (1, 10, 128):
        val, idx = ref.topk_ref(s, k)
        st = torch.sort(torch.from_numpy(s), dim=1, descending=True)
        assert np.array_equal(idx, st.indices[:, :k].numpy())
        assert np.array_equal(val.view(np.uint32), st.values[:, :k].numpy().view(np.uint32))


def test_restatement_ties_filters_padding():
    s = np.array([[1.0, 2.0, 2.0, -0.0, 0.0, np.nan, -np.inf, 2.0]], dtype=np.float32)
    val, idx = ref.topk_ref(s, 10, col_begin=100)
    assert idx.tolist() == [[101, 102, 107, 100, 103, 104, 105, 106, -1, -1]]
    assert val[0, 4] == 0 and not np.signbit(val[0, 4]) and not np.signbit(val[0, 5])  # -0.0 came out as +0.0
    assert np.all(np.isneginf(val[0, 6:]))
    f = [(np.array([0]), np.array([4]), np.array([101, 102, 5, 100]))]  # 5: outside the slice, ignored
    val, idx = ref.topk_ref(s, 3, filters=f, keep=np.array([102]), col_begin=100)
    assert idx.tolist() == [[102, 107, 103]]


SPECIAL = np.array([-np.inf, -3.0e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.17549435e-38, 2.0 ** -126, 1.0, 3.0e38, np.inf],
                   dtype=np.float32)


def test_key_packing_is_monotone_and_round_trips():
    vals = np.concatenate([SPECIAL, np.array([np.nan], dtype=np.float32)])
    keys = ref.pack_keys(vals, np.full(len(vals), 7))
    hi = (keys >> np.uint64(32)).astype(np.int64)
    canon = ref.canonical(vals)
    for a in range(len(vals)):
        for b in range(len(vals)):
            assert (hi[a] < hi[b]) == (canon[a] < canon[b]), (vals[a], vals[b])
            assert (hi[a] == hi[b]) == (canon[a] == canon[b]), (vals[a], vals[b])
    assert np.all(keys != 0)
    # equal scores: the smaller column has the larger key; the largest admissible column still has a non-zero key
    k2 = ref.pack_keys(np.array([1.0, 1.0, -np.inf], dtype=np.float32), np.array([3, 4, 2 ** 32 - 2]))
    assert k2[0] > k2[1] and k2[2] != 0
    v, j = ref.unpack_keys(keys, col_begin=5)
    assert np.array_equal(v.view(np.uint32), canon.view(np.uint32))
    assert np.all(j == 12)
    v0, j0 = ref.unpack_keys(np.zeros(2, dtype=np.uint64))
    assert np.all(np.isneginf(v0)) and np.all(j0 == -1)


@pytest.mark.parametrize("k", [1, 10, 64, 128])
def test_merging_group_lists_of_any_split_equals_the_one_group_result(k):
    rng = np.random.default_rng(k)
    n, m = 5, 333
    s = rng.integers(-3, 4, size=(n, m)).astype(np.float32)  # many ties
    s[1, 17] = np.nan
    s[2, 200] = -np.inf
    s[3, :] = 1.0
    begin = np.array([0, 3, 3, 3, 3])
    end = np.array([3, 3, 3, 3, 3 + m])
    col = np.concatenate([[5, 64, 900], np.arange(m)]).astype(np.int64)  # row 4: every column removed
    filters = [(begin, end, col)]
    want = ref.topk_ref(s, k, filters)
    assert np.all(want[1][4] == -1)
    for cuts in ([], [64], [64, 128, 192, 256, 320], [1, 2, 3, 332], sorted(rng.choice(m, 20, replace=False).tolist())):
        got = ref.topk_by_groups(s, k, cuts, filters)
        assert np.array_equal(got[1], want[1]), cuts
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), cuts


@pytest.mark.parametrize("name", ["complex", "distmult", "transe", "rotate"])
def test_cpu_fallback_of_predict_equals_the_restatement(name, monkeypatch):
    """A model on CPU parameters takes the torch composition.  (The composed score itself has no CPU path: score_sp /
    score_po are replaced by recorded stand-ins -- small integers, so every row has equal scores, plus non-finite ones
    -- and the result must be the restatement on exactly what they returned.)"""
    from kge_amd import model as M
    from kge_amd.eval import FilterIndex
    from kge_amd.synthetic import make_splits
    E, R, d, n = 97, 5, 8, 23
    ds = make_splits(E, R, 400, 60, 60, seed=3)
    fi = FilterIndex([ds["train"], ds["valid"]], E, R)
    mdl = M.create(name, E, R, d)
    g = torch.Generator().manual_seed(1)
    sc_sp = torch.randint(-3, 4, (n, E), generator=g).float()
    sc_po = torch.randint(-3, 4, (n, E), generator=g).float()
    sc_sp[0, 5], sc_sp[1, 9], sc_sp[2, 11], sc_po[3, 0] = float("nan"), float("-inf"), -0.0, float("inf")
    monkeypatch.setattr(mdl, "score_sp", lambda s_, p_, o_=None: sc_sp)
    monkeypatch.setattr(mdl, "score_po", lambda p_, o_, s_=None: sc_po)
    tri = torch.from_numpy(ds["valid"][:n].astype(np.int64))
    s, p, o = tri[:, 0], tri[:, 1], tri[:, 2]
    sb, se, pb, pe = fi.ranges(tri.numpy())
    for k in (1, 10, 128):
        for keep in (None, o):
            val, idx = mdl.predict_o(s, p, k, fi, keep)
            want = ref.topk_ref(mdl.score_sp(s, p).detach().numpy(), k, [(sb, se, fi.sp_values)],
                                None if keep is None else keep.numpy())
            assert val.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(idx.shape) == (n, k)
            assert np.array_equal(idx.numpy(), want[1])
            assert np.array_equal(val.numpy().view(np.uint32), want[0].view(np.uint32))
        val, idx = mdl.predict_s(p, o, k, fi, s)
        want = ref.topk_ref(mdl.score_po(p, o).detach().numpy(), k, [(pb, pe, fi.po_values)], s.numpy())
        assert np.array_equal(idx.numpy(), want[1])
        assert np.array_equal(val.numpy().view(np.uint32), want[0].view(np.uint32))
    val, idx = mdl.predict_o(s, p, 7)  # no filter index
    want = ref.topk_ref(mdl.score_sp(s, p).detach().numpy(), 7)
    assert np.array_equal(idx.numpy(), want[1])


def test_engine_topk_rejects_bad_arguments_before_any_library_call(monkeypatch):
    from kge_amd import _lib, engine

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(engine, "_ext", no_library)
    ix = torch.zeros(3, dtype=torch.int64)
    assert _lib.TOPK_MAX >= 128
    for k in (0, -1, _lib.TOPK_MAX + 1, 1.5, True):
        with pytest.raises(ValueError, match="k must be"):
            engine.topk(None, "sp_", ix, ix, k)
    with pytest.raises(ValueError, match="direction"):
        engine.topk(None, "spo", ix, ix, 3)
    bad = [[(ix, ix)], [ix], [(ix, ix, None)], [(ix, ix, ix.int())], [(ix, ix[:2], ix)], [(ix, ix, ix)] * 3,
           [(ix, ix, ix.reshape(3, 1))]]
    for f in bad:
        with pytest.raises(ValueError, match="filter"):
            engine.topk(None, "sp_", ix, ix, 3, filters=f)
