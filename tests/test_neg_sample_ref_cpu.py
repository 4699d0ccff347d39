"""tests/_neg_sample_ref.py -- the numpy restatement of kge_neg_sample that the GPU tests compare bits with -- checked on
its own, without a GPU: Philox4x32-10 against the Random123 known-answer vectors, the sampler's semantics against what
the reference's sampler guarantees (kge/util/sampler.py:80-137, 163-196), and its distributions against their laws.

Distribution bound: a chi-square statistic over df = (cells - 1) degrees of freedom has mean df and variance 2 df; the
tests ask for at most df + 5 sqrt(2 df) at one fixed seed (deterministic: the draws are counter based)."""
import os

import numpy as np
import pytest

import _neg_sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = " ".join("%08x" % int(x) for x in R.philox4x32_10(*ctr, *key))
    assert got == want


def test_philox_is_vectorised_elementwise():
    c = np.arange(7, dtype=np.uint64)
    vec = R.philox4x32_10(c, 3, c[::-1], 9, 11, 13)
    for j in range(7):
        one = R.philox4x32_10(int(c[j]), 3, int(c[6 - j]), 9, 11, 13)
        assert [int(v[j]) for v in vec] == [int(v) for v in one]


def test_umul64hi_against_python_integers():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 64, size=200, dtype=np.uint64)
    x[:3] = [0, 1, 2 ** 64 - 1]
    for v in (1, 2, 7, 1000, 2 ** 31 + 11, 2 ** 63 - 1):
        assert [int(h) for h in R.umul64hi(x, v)] == [(int(a) * v) >> 64 for a in x]


def _graph(n, vocab, seed, max_pos):
    """n rows with keys a * 1000 + b; each key with 0..max_pos known answers."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 9, n), rng.integers(0, 5, n)
    keys, vals = [], []
    for key in np.unique(a * 1000 + b):
        m = int(rng.integers(0, max_pos + 1))
        v = rng.choice(vocab, size=min(m, vocab), replace=False)
        keys += [key] * len(v)
        vals += list(v)
    return a, b, R.build_index(keys, vals, vocab)


def _positives_of(index, a, b, mult, i):
    begin, end = R.key_ranges(index, np.asarray(a) * mult + np.asarray(b))
    return set(int(v) for v in index[2][begin[i]:end[i]])


@pytest.mark.parametrize("vocab,max_pos", [(50, 20), (7, 7), (1000, 300)])
@pytest.mark.parametrize("alias", [False, True])
def test_restatement_has_the_reference_samplers_semantics(vocab, max_pos, alias):
    n, K, slot, seed, call = 23, 70, 2, 0x1234567890ABCDEF, 5
    a, b, index = _graph(n, vocab, 1, max_pos)
    al = R.alias_setup(np.arange(1, vocab + 1, dtype=np.float64)) if alias else None
    plain, st0, att0 = R.sample(n, K, vocab, slot, seed, call, alias=al)
    filt, st, att = R.sample(n, K, vocab, slot, seed, call, alias=al, index=index, a=a, b=b, mult=1000)
    assert plain.shape == filt.shape == (n, K) and plain.dtype == np.int64
    assert plain.min() >= 0 and plain.max() < vocab and filt.min() >= 0 and filt.max() < vocab
    assert not st0.any() and not att0.any()
    first_was_positive = np.zeros((n, K), dtype=bool)
    for i in range(n):
        pos = _positives_of(index, a, b, 1000, i)
        first_was_positive[i] = [int(x) in pos for x in plain[i]]
        bad = np.array([int(x) in pos for x in filt[i]])
        # no sample is a training answer of its row's key, unless the row's stats count it as capped
        assert bad.sum() == st[i, 1], (i, bad.sum(), st[i])
        if len(pos) < vocab and not alias:
            assert st[i, 1] == 0  # (uniform over a vocabulary with a free id: 256 rejections in a row do not happen here)
    # unfiltered output = filtered output wherever the first draw was not a positive
    assert np.array_equal(plain[~first_was_positive], filt[~first_was_positive])
    assert np.array_equal(att == 0, ~first_was_positive)
    # a filtered position holds the restatement's draw of its attempt t >= 1
    rows, cols = np.nonzero(first_was_positive)
    assert (att[rows, cols] >= 1).all()
    again = R.draw(rows, cols, att[rows, cols], vocab, slot, seed, call, al)
    assert np.array_equal(again, filt[rows, cols])
    # stats: the rejected attempts of a row are its positions' attempt numbers (+1 for a capped position's kept draw)
    capped = att == R.MAX_ATTEMPTS - 1
    for i in range(n):
        pos = _positives_of(index, a, b, 1000, i)
        kept_bad = np.array([int(x) in pos for x in filt[i]])
        assert st[i, 0] == att[i].sum() + (capped[i] & kept_bad).sum()


def test_restatement_row_with_the_whole_vocabulary_known_is_capped_and_returns():
    vocab, K = 8, 5
    index = R.build_index([3] * vocab + [4] * (vocab - 1), list(range(vocab)) + [0, 1, 2, 3, 4, 6, 7], vocab)
    out, st, att = R.sample(3, K, vocab, 0, 1, 0, index=index, a=[0, 0, 0], b=[3, 4, 5], mult=10)
    assert st[0, 1] == K and st[0, 0] == K * R.MAX_ATTEMPTS and (att[0] == R.MAX_ATTEMPTS - 1).all()
    assert (out[1] == 5).all() and st[1, 1] == 0  # all but one id known: every sample is that id
    assert st[2].tolist() == [0, 0]               # key absent from the index: the first draws


def test_seed_call_slot_row_and_column_all_enter_the_draw():
    base = R.sample(4, 6, 10 ** 6, 0, 7, 3)[0]
    assert np.array_equal(base, R.sample(4, 6, 10 ** 6, 0, 7, 3)[0])
    for other in (R.sample(4, 6, 10 ** 6, 2, 7, 3)[0], R.sample(4, 6, 10 ** 6, 0, 8, 3)[0],
                  R.sample(4, 6, 10 ** 6, 0, 7 + 2 ** 32, 3)[0], R.sample(4, 6, 10 ** 6, 0, 7, 4)[0]):
        assert not np.array_equal(base, other)
    assert len(np.unique(base)) == base.size  # (24 draws from 10^6 ids: rows and columns differ)
    # a larger launch draws the same numbers at the shared positions
    assert np.array_equal(R.sample(9, 11, 10 ** 6, 0, 7, 3)[0][:4, :6], base)


def _chi2(counts, law):
    total = counts.sum()
    expect = law * total
    return float(((counts - expect) ** 2 / expect).sum())


SEED = 20261019


def test_uniform_distribution():
    vocab, n, K = 50, 200, 1000
    out, _, _ = R.sample(n, K, vocab, 0, SEED, 0)
    stat = _chi2(np.bincount(out.reshape(-1), minlength=vocab), np.full(vocab, 1.0 / vocab))
    df = vocab - 1
    print(f"uniform chi2 {stat:.2f} df {df} bound {df + 5 * np.sqrt(2 * df):.2f}")
    assert stat <= df + 5 * np.sqrt(2 * df)


def test_frequency_distribution():
    vocab, n, K = 50, 200, 1000
    counts = (np.arange(vocab) % 7) ** 3 + np.arange(vocab) // 10  # skewed, with zero counts
    smoothed = counts + 1.0
    law = smoothed / smoothed.sum()
    alias = R.alias_setup(law)
    assert np.abs(R.alias_law(*alias) - law).max() < 1e-7  # (the tables, float32 probabilities included, hold the law)
    out, _, _ = R.sample(n, K, vocab, 2, SEED, 1, alias=alias)
    stat = _chi2(np.bincount(out.reshape(-1), minlength=vocab), law)
    df = vocab - 1
    print(f"frequency chi2 {stat:.2f} df {df} bound {df + 5 * np.sqrt(2 * df):.2f}")
    assert stat <= df + 5 * np.sqrt(2 * df)


def test_filtered_uniform_distribution():
    vocab, n, K = 50, 200, 1000
    excluded = np.arange(0, 40, 2)  # the row's 20 positives
    index = R.build_index([11] * 20, excluded, vocab)
    out, st, _ = R.sample(n, K, vocab, 2, SEED, 2, index=index, a=np.ones(n, np.int64), b=np.ones(n, np.int64), mult=10)
    cnt = np.bincount(out.reshape(-1), minlength=vocab)
    assert cnt[excluded].sum() == 0 and st[:, 1].sum() == 0
    free = np.setdiff1d(np.arange(vocab), excluded)
    stat = _chi2(cnt[free], np.full(30, 1.0 / 30))
    df = 29
    print(f"filtered uniform chi2 {stat:.2f} df {df} bound {df + 5 * np.sqrt(2 * df):.2f}")
    assert stat <= df + 5 * np.sqrt(2 * df)


def test_abi_prototype_is_declared():
    import ctypes
    from kge_amd import _lib
    res, args = _lib.PROTOTYPES["kge_neg_sample"]
    assert res is ctypes.c_int and len(args) == 19
    assert args[4] is ctypes.c_uint64 and args[5] is ctypes.c_uint64 and args[12] is _lib.KgeIndex and args[13] is _lib.KgeIndex
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    assert "int kge_neg_sample(" in header and "#define KGE_NEG_SAMPLE_MAX_ATTEMPTS 256" in header
    assert R.MAX_ATTEMPTS == 256


def test_yaml_option_exists_and_is_false_by_default():
    import yaml
    with open(os.path.join(ROOT, "kge_amd", "libkge_plugin", "hip_negative_sampling.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["hip_negative_sampling"]["device_sampler"] is False


def test_device_sampler_is_a_public_name_and_matches_the_restatements_alias_tables():
    import kge_amd
    from kge_amd.sampler import DeviceSampler, alias_setup
    assert kge_amd.DeviceSampler is DeviceSampler and "DeviceSampler" in kge_amd.__all__
    law = np.array([0.1, 0.2, 0.3, 0.05, 0.35])
    p0, i0 = alias_setup(law)
    p1, i1 = R.alias_setup(law)
    assert np.array_equal(p0, p1) and np.array_equal(i0, i1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceSampler(np.zeros((1, 3), dtype=np.int64), 4, 2, device="cpu")
