"""kge_neg_sample on the MI355X against its numpy restatement (tests/_neg_sample_ref.py), bit for bit: the samples
are integers from a counter-based generator, so there is no tolerance anywhere in this file -- `out` and `stats` are
compared with array_equal.  Shapes: one column, fewer columns than lanes, exactly 64, 65 (a second pass of the wave with
one live lane) and 200; one row, rows that do not fill a block of four waves, many blocks."""
import itertools

import numpy as np
import pytest
import torch

import _neg_sample_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 5, 64, 257)
KS = (1, 3, 64, 65, 200)
VOCABS = (1, 2, 7, 1000, 2 ** 31 + 11)
SEED_CALLS = ((0x9E3779B97F4A7C15, 0), (3, 2 ** 32 + 5))  # (a 64-bit seed; a call number past 32 bits wraps in the counter)
SENTINEL = -7
MULT = 1000


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _to(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _index_of(t):
    from kge_amd import _lib
    return _lib.KgeIndex(t.data_ptr(), _lib.I32 if t.dtype == torch.int32 else _lib.I64, 0, t.stride(0) if t.numel() > 1 else 1)


def _raw(dev, n, K, vocab, slot, seed, call, alias=None, index=None, a=None, b=None, mult=0, pad=0, i32=False,
         want_stats=True):
    """The C entry point through ctypes -> (the whole [n, K + pad] buffer, stats [n, 2]); the status must be KGE_OK."""
    from kge_amd import _lib
    out = torch.full((n, K + pad), SENTINEL, dtype=torch.int64, device=dev)
    stats = torch.full((n, 2), SENTINEL, dtype=torch.int32, device=dev)
    keep = []
    ap = ai = keys = starts = values = None
    num_keys = 0
    ia = ib = _lib.KgeIndex(None, _lib.I64, 0, 1)
    if alias is not None:
        keep += [_to(alias[0], dev), _to(alias[1], dev)]
        ap, ai = keep[-2].data_ptr(), keep[-1].data_ptr()
    if index is not None:
        vals = index[2] if len(index[2]) else np.zeros(1, np.int64)
        keep += [_to(index[0], dev), _to(index[1], dev), _to(vals, dev)]
        keys, starts, values = (t.data_ptr() for t in keep[-3:])
        num_keys = len(index[0])
        ab = _to(np.stack([a, b], 1), dev, torch.int32 if i32 else torch.int64)  # [n, 2]: the columns have stride 2
        keep.append(ab)
        ia, ib = _index_of(ab[:, 0]), _index_of(ab[:, 1])
    with torch.cuda.device(dev):
        rc = _lib.lib().kge_neg_sample(n, K, vocab, slot, seed, call, ap, ai, keys, num_keys, starts, values, ia, ib, mult,
                                       out.data_ptr(), K + pad, stats.data_ptr() if want_stats else None,
                                       torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), stats.cpu().numpy()


def _keys_and_index(n, K, vocab, slot, seed, call, alias, salt):
    """Rows over ~45 keys; a key's known answers are random ids plus some of its rows' own first draws (so that the filter
    fires at every vocabulary size); some keys are not in the index, some have all ids but one or a long range."""
    rng = np.random.default_rng(1000 + salt)
    a, b = rng.integers(0, 9, n), rng.integers(0, 5, n)
    plain = R.sample(n, K, vocab, slot, seed, call, alias=alias)[0]
    keys, vals = [], []
    for j, key in enumerate(np.unique(a * MULT + b)):
        if j % 3 == 2 or (vocab <= 2 and j % 6):
            continue  # a key of the batch that the index does not hold (vocab 1, 2: most keys -- their rows run to the cap)
        rows = np.nonzero(a * MULT + b == key)[0]
        v = list(plain[rows[0], :2]) + list(rng.integers(0, vocab, 3))
        if j % 7 == 0 and 1 < vocab <= 7:
            v = list(range(vocab - 1))  # all ids but the last
        elif j % 7 == 0 and vocab == 1000:
            v = list(rng.choice(vocab, 900, replace=False))  # a long range: nine draws in ten are rejected
        keys += [key] * len(v)
        vals += v
    keys += [10 ** 7]  # a key past every row's
    vals += [0]
    return a, b, R.build_index(keys, vals, vocab)


@pytest.mark.parametrize("vocab", VOCABS)
def test_bits_equal_the_restatement(dev, vocab):
    checked = {"filtered": 0, "rejected": 0, "capped": 0}
    for c, (n, K) in enumerate(itertools.product(NS, KS)):
        for flip in (0, 1):
            bit = lambda j: ((c >> j) & 1) ^ flip
            slot = (0, 2)[bit(0)]
            seed, call = SEED_CALLS[bit(1)]
            filtered, pad, i32 = bool(bit(2)), (0, 3)[bit(3)], bool(bit(4))
            alias = None
            if vocab <= 1000 and ((c // 2 + flip) & 1):
                alias = R.alias_setup(np.arange(1, vocab + 1, dtype=np.float64) ** 2)
            kw = {}
            if filtered:
                a, b, index = _keys_and_index(n, K, vocab, slot, seed, call, alias, c)
                kw = dict(index=index, a=a, b=b, mult=MULT)
            want, wstats, _ = R.sample(n, K, vocab, slot, seed, call, alias=alias, **kw)
            got, gstats = _raw(dev, n, K, vocab, slot, seed, call, alias=alias, pad=pad, i32=i32, **kw)
            what = (n, K, vocab, slot, seed, call, alias is not None, filtered, pad, i32)
            assert np.array_equal(got[:, :K], want), what
            assert np.array_equal(gstats, wstats), what
            assert (got[:, K:] == SENTINEL).all(), what  # the padding columns of ld = K + 3 are untouched
            assert got[:, :K].min() >= 0 and got[:, :K].max() < vocab
            checked["filtered"] += filtered
            checked["rejected"] += int(wstats[:, 0].sum())
            checked["capped"] += int(wstats[:, 1].sum())
    print(f"vocab {vocab}: {checked}")
    assert checked["filtered"] == len(NS) * len(KS) and checked["rejected"] > 0
    if vocab == 1:
        assert checked["capped"] > 0  # (the only id is a known answer: every such column runs into the cap)


def _manual_index(entries):
    """entries: [(key, [values])], keys ascending; an empty list is a key with an EMPTY range."""
    keys = np.array([k for k, _ in entries], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum([len(v) for _, v in entries])]).astype(np.int64)
    values = np.array([x for _, v in entries for x in sorted(v)], dtype=np.int64)
    return keys, starts, values


def test_filter_edges(dev):
    vocab, K = 8, 70
    index = _manual_index([(2, [1]),                       # the first key: a range of length 1
                           (5, []),                        # a key with an empty range
                           (7, [0, 1, 2, 3, 4, 6, 7]),     # all ids but 5
                           (9, list(range(8))),            # the whole vocabulary
                           (11, [3, 4])])                  # the last key
    b = np.array([4, 2, 5, 7, 9, 11, 7, 12], dtype=np.int64)  # 4 and 12: keys the index does not hold
    a = np.zeros(len(b), dtype=np.int64)
    n = len(b)
    for slot, (seed, call) in itertools.product((0, 2), SEED_CALLS):
        want, wstats, _ = R.sample(n, K, vocab, slot, seed, call, index=index, a=a, b=b, mult=MULT)
        plain = R.sample(n, K, vocab, slot, seed, call)[0]
        got, gstats = _raw(dev, n, K, vocab, slot, seed, call, index=index, a=a, b=b, mult=MULT)
        assert np.array_equal(got, want) and np.array_equal(gstats, wstats)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[7], plain[7]) and not gstats[[0, 7]].any()  # absent
        assert np.array_equal(got[2], plain[2]) and not gstats[2].any()   # empty range
        assert (got[1] != 1).all() and gstats[1, 1] == 0                  # first key, one known answer
        assert (got[3] == 5).all() and (got[6] == 5).all() and gstats[3, 1] == 0 and gstats[6, 1] == 0
        assert gstats[4, 1] == K and gstats[4, 0] == K * R.MAX_ATTEMPTS    # the whole vocabulary: capped, and it returned
        assert not np.isin(got[5], [3, 4]).any() and gstats[5, 1] == 0    # last key
        # the rows beside the capped one are what they are without it
        keep = np.array([0, 1, 2, 3, 5, 6, 7])
        w2 = R.sample(n, K, vocab, slot, seed, call, index=_manual_index([e for e in
                      [(2, [1]), (5, []), (7, [0, 1, 2, 3, 4, 6, 7]), (11, [3, 4])]]), a=a, b=b, mult=MULT)[0]
        assert np.array_equal(got[keep], w2[keep])


def test_long_and_short_ranges_in_a_large_vocabulary(dev):
    vocab, n, K = 6000, 6, 130
    rng = np.random.default_rng(5)
    long_range = np.sort(rng.choice(vocab, 5000, replace=False))
    index = _manual_index([(1, [4321]), (3, list(long_range))])
    a, b = np.zeros(n, dtype=np.int64), np.array([3, 1, 3, 2, 1, 3], dtype=np.int64)
    want, wstats, _ = R.sample(n, K, vocab, 2, 11, 1, index=index, a=a, b=b, mult=MULT)
    got, gstats = _raw(dev, n, K, vocab, 2, 11, 1, index=index, a=a, b=b, mult=MULT, i32=True)
    assert np.array_equal(got, want) and np.array_equal(gstats, wstats)
    for i in (0, 2, 5):
        assert not np.isin(got[i], long_range).any() and gstats[i, 0] > K and gstats[i, 1] == 0  # (5 of 6 draws rejected)
    assert (got[[1, 4]] != 4321).all()


def test_determinism_and_what_enters_the_draw(dev):
    n, K, vocab = 37, 90, 10 ** 6
    base, _ = _raw(dev, n, K, vocab, 0, 42, 7)
    again, _ = _raw(dev, n, K, vocab, 0, 42, 7)
    assert np.array_equal(base, again)
    assert not np.array_equal(base, _raw(dev, n, K, vocab, 0, 42, 8)[0])   # call + 1
    assert not np.array_equal(base, _raw(dev, n, K, vocab, 2, 42, 7)[0])   # the other slot
    assert not np.array_equal(base, _raw(dev, n, K, vocab, 0, 43, 7)[0])   # another seed
    # a smaller launch draws the same numbers at the shared positions (no dependence on the launch geometry)
    assert np.array_equal(_raw(dev, 5, 3, vocab, 0, 42, 7)[0], base[:5, :3])
    # without a stats pointer nothing is written there and the samples are the same
    out, stats = _raw(dev, n, K, vocab, 0, 42, 7, want_stats=False)
    assert np.array_equal(out, base) and (stats == SENTINEL).all()


def test_limits_and_invalid_arguments(dev):
    from kge_amd import _lib
    L = _lib.lib()
    none = _lib.KgeIndex(None, _lib.I64, 0, 1)
    buf = torch.full((4, 4), SENTINEL, dtype=torch.int64, device=dev)
    f32 = torch.ones(4, device=dev)
    i64 = torch.zeros(5, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(n=4, K=4, vocab=4, slot=0, ap=None, ai=None, keys=None, starts=None, values=None, a=none, b=none, out=buf, ld=4):
        with torch.cuda.device(dev):
            return L.kge_neg_sample(n, K, vocab, slot, 1, 0, ap, ai, keys, 0 if keys is None else 1, starts, values, a, b, 10,
                                    None if out is None else out.data_ptr(), ld, None, st)

    assert call(n=0) == 0 and call(K=0) == 0 and call(n=0, out=None) == 0
    torch.cuda.synchronize(dev)
    assert (buf == SENTINEL).all()  # nothing written
    assert call(vocab=0) == -1 and call(vocab=-3) == -1
    assert call(slot=1) == -1 and call(slot=3) == -1 and call(slot=-1) == -1
    assert call(ap=f32.data_ptr()) == -1 and call(ai=i64.data_ptr()) == -1          # half an alias table
    assert call(keys=i64.data_ptr()) == -1                                           # keys without starts / values
    assert call(keys=i64.data_ptr(), starts=i64.data_ptr(), values=i64.data_ptr()) == -1   # ... without a / b
    assert call(ld=3) == -1 and call(out=None) == -1 and call(n=-1) == -1
    torch.cuda.synchronize(dev)
    assert (buf == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert int(buf.min()) >= 0 and int(buf.max()) < 4


def test_engine_and_extension_agree_with_the_ctypes_path(dev):
    from kge_amd import _lib, engine
    n, K, vocab, slot, seed, call = 33, 65, 1000, 2, 99, 4
    alias = R.alias_setup(np.arange(1, vocab + 1, dtype=np.float64))
    a, b, index = _keys_and_index(n, K, vocab, slot, seed, call, alias, 77)
    raw, raw_stats = _raw(dev, n, K, vocab, slot, seed, call, alias=alias, index=index, a=a, b=b, mult=MULT)
    al = (_to(alias[0], dev), _to(alias[1], dev))
    ix = tuple(_to(x, dev) for x in index)
    ta, tb = _to(a, dev), _to(b, dev, torch.int32)
    # engine.neg_sample: the extension when it is built (no out given), else ctypes
    out, stats = engine.neg_sample(n, K, vocab, slot, seed, call, alias=al, index=ix, a=ta, b=tb, mult=MULT, stats=True)
    assert out.dtype == torch.int64 and out.is_cuda and tuple(out.shape) == (n, K) and stats.dtype == torch.int32
    assert np.array_equal(out.cpu().numpy(), raw) and np.array_equal(stats.cpu().numpy(), raw_stats)
    # ... into a slice of a wider matrix: the ctypes path of the engine
    wide = torch.full((n, K + 3), SENTINEL, dtype=torch.int64, device=dev)
    st2 = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    out2, st2b = engine.neg_sample(n, K, vocab, slot, seed, call, alias=al, index=ix, a=ta, b=tb, mult=MULT,
                                   out=wide[:, :K], stats=st2)
    assert out2.data_ptr() == wide.data_ptr() and st2b is st2
    assert np.array_equal(wide[:, :K].cpu().numpy(), raw) and (wide[:, K:] == SENTINEL).all()
    assert np.array_equal(st2.cpu().numpy(), raw_stats)
    # the _C binding itself
    ex = _lib.ext()
    o3, s3 = ex.neg_sample(ta, n, K, vocab, slot, seed, call, al[0], al[1], ix[0], ix[1], ix[2], ta, tb, MULT, True)
    assert np.array_equal(o3.cpu().numpy(), raw) and np.array_equal(s3.cpu().numpy(), raw_stats)
    o4, s4 = ex.neg_sample(ta, n, K, vocab, slot, seed, call, None, None, None, None, None, None, None, 0, False)
    assert s4 is None and np.array_equal(o4.cpu().numpy(), R.sample(n, K, vocab, slot, seed, call)[0])
    # uniform, unfiltered, without statistics: a tensor alone
    plain = engine.neg_sample(n, K, vocab, slot, seed, call, device=dev)
    assert torch.is_tensor(plain) and np.array_equal(plain.cpu().numpy(), o4.cpu().numpy())
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.neg_sample(n, K, vocab, slot, seed, call, device="cpu")


@pytest.mark.parametrize("sampling_type", ["uniform", "frequency"])
def test_device_sampler_on_a_synthetic_graph(dev, sampling_type):
    from kge_amd import DeviceSampler
    from kge_amd.sampler import alias_setup
    E, Rn, N, K = 40, 3, 300, 50
    rng = np.random.default_rng(8)
    tri = np.stack([rng.integers(0, E, N), rng.integers(0, Rn, N), rng.integers(0, E, N)], 1).astype(np.int64)
    known = set(map(tuple, tri.tolist()))
    smp = DeviceSampler(tri, E, Rn, sampling_type=sampling_type, smoothing=1.0, filter_s=True, filter_o=True, seed=123,
                        device=dev)
    assert smp.last_stats is None and smp.calls == 0
    batch = torch.from_numpy(tri[:64]).to(dev)
    for call, slot in enumerate((0, 2, 0)):
        out = smp.sample(batch, slot, K)
        assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (64, K) and smp.calls == call + 1
        got, stats = out.cpu().numpy(), smp.last_stats.cpu().numpy()
        assert stats[:, 1].sum() == 0  # (a key of this graph knows a few of the 40 entities: nothing runs into the cap)
        for i, (s, p, o) in enumerate(tri[:64]):
            for x in got[i]:
                assert ((int(x), p, o) if slot == 0 else (s, p, int(x))) not in known
        # the restatement on its own index of the same triples, its own alias tables, the sampler's seed and call number
        if slot == 0:
            index, a, b, mult = R.build_index(tri[:, 1] * E + tri[:, 2], tri[:, 0], E), tri[:64, 1], tri[:64, 2], E
        else:
            index, a, b, mult = R.build_index(tri[:, 0] * Rn + tri[:, 1], tri[:, 2], E), tri[:64, 0], tri[:64, 1], Rn
        alias = None
        if sampling_type == "frequency":
            smoothed = np.bincount(tri[:, slot], minlength=E) + 1.0
            alias = R.alias_setup(smoothed / smoothed.sum())
        want, wstats, _ = R.sample(64, K, E, slot, 123, call, alias=alias, index=index, a=a, b=b, mult=mult)
        assert np.array_equal(got, want)
        assert stats[:, 0].sum() == wstats[:, 0].sum() and stats[:, 1].sum() == wstats[:, 1].sum()
        assert stats[:, 0].sum() > 0
    with pytest.raises(ValueError):
        smp.sample(batch, 1, K)
