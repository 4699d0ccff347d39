"""numpy restatement of kge_neg_sample (include/kge_amd.h; kge_amd/csrc/neg_sample.hip): Philox4x32-10 and the whole
sampler -- draw, alias, filter, cap, stats -- in vectorised uint64 arithmetic.  No torch, no GPU.

Layout restated (the header documents the same):
  key     = (seed low 32, seed high 32)
  counter = (k, i, t, (uint32)call * 4 + slot)      one Philox block r0..r3 per (row i, column k, attempt t)
  uniform   id = umul64hi((r0 << 32) | r1, vocab)
  frequency bucket = umul64hi((r0 << 32) | r1, vocab), u = (r2 >> 8) * 2^-24 (float32),
            id = u < alias_prob[bucket] ? bucket : alias_idx[bucket]
  out[i, k] = the draw of the first attempt t that is not a known answer of row i's key a[i] * mult + b[i]; after
  MAX_ATTEMPTS rejected attempts the column keeps its last draw.
  stats[i] = (rejected attempts of the row, the kept draw of a capped column included; columns that hit the cap)
"""
import numpy as np

MAX_ATTEMPTS = 256
_M32 = np.uint64(0xFFFFFFFF)
_PM0, _PM1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counter words (arrays or scalars, broadcast together) under the key (k0, k1):
    -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _PM0 * c0, _PM1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return c0, c1, c2, c3


def umul64hi(x, v):
    """High 64 bits of the 128-bit product of uint64 array x and the scalar v (< 2^64)."""
    x = np.asarray(x, dtype=np.uint64)
    v = int(v)
    vl, vh = np.uint64(v & 0xFFFFFFFF), np.uint64(v >> 32)
    xl, xh = x & _M32, x >> _S32
    ll, lh, hl, hh = xl * vl, xl * vh, xh * vl, xh * vh
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def draw(rows, cols, t, vocab, slot, seed, call, alias=None):
    """The draw of attempt t (scalar or array) at (rows, cols): int64 ids in [0, vocab)."""
    seed, call = int(seed) & (2 ** 64 - 1), int(call)
    c3 = ((call & 0xFFFFFFFF) * 4 + int(slot)) & 0xFFFFFFFF
    r0, r1, r2, _ = philox4x32_10(cols, rows, t, c3, seed & 0xFFFFFFFF, seed >> 32)
    ids = umul64hi((r0 << _S32) | r1, vocab).astype(np.int64)
    if alias is not None:
        prob, idx = alias
        u = (r2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        ids = np.where(u < np.asarray(prob, dtype=np.float32)[ids], ids, np.asarray(idx, dtype=np.int64)[ids])
    return ids


def key_ranges(index, keys):
    """index = (sorted_keys, starts, values) -> per key its [begin, end) in values ((0, 0) for an absent key)."""
    uk, starts, _ = index
    keys = np.asarray(keys, dtype=np.int64)
    if len(uk) == 0:
        z = np.zeros(len(keys), dtype=np.int64)
        return z, z.copy()
    pos = np.minimum(np.searchsorted(uk, keys), len(uk) - 1)
    hit = uk[pos] == keys
    return np.where(hit, starts[pos], 0).astype(np.int64), np.where(hit, starts[pos + 1], 0).astype(np.int64)


def _pair_table(index, vocab):
    """(key position, value) of every index entry as one sorted int64 array: position * vocab + value."""
    uk, starts, values = (np.asarray(x, dtype=np.int64) for x in index)
    assert len(uk) * int(vocab) < 2 ** 62
    return np.repeat(np.arange(len(uk), dtype=np.int64), np.diff(starts)) * int(vocab) + values[:starts[-1]]


def is_positive(pairs, kpos, vocab, rows, ids):
    """Is ids[j] a known answer of row rows[j]'s key (kpos[row] = the key's position in the index, -1 if absent)?"""
    if len(pairs) == 0:
        return np.zeros(len(ids), dtype=bool)
    want = kpos[rows] * int(vocab) + ids
    p = np.minimum(np.searchsorted(pairs, want), len(pairs) - 1)
    return (kpos[rows] >= 0) & (pairs[p] == want)


def sample(n, K, vocab, slot, seed, call, alias=None, index=None, a=None, b=None, mult=0, max_attempts=MAX_ATTEMPTS,
           first_attempt=0):
    """-> (out int64 [n, K], stats int32 [n, 2], attempts int64 [n, K]: the attempt whose draw each position holds).
    first_attempt > 0 starts the sequence later (tests: "a filtered position is the restatement's attempt t >= 1")."""
    rows, cols = [x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(K), indexing="ij")]
    out = np.zeros(n * K, dtype=np.int64)
    att = np.zeros(n * K, dtype=np.int64)
    stats = np.zeros((n, 2), dtype=np.int32)
    if n * K == 0:
        return out.reshape(n, K), stats, att.reshape(n, K)
    if index is not None:
        keys = np.asarray(a, dtype=np.int64) * int(mult) + np.asarray(b, dtype=np.int64)
        uk = np.asarray(index[0], dtype=np.int64)
        kpos = np.full(n, -1, dtype=np.int64)
        if len(uk):
            p = np.minimum(np.searchsorted(uk, keys), len(uk) - 1)
            kpos = np.where(uk[p] == keys, p, -1)
        pairs = _pair_table(index, vocab)
    active = np.arange(n * K)
    t = first_attempt
    while len(active):
        ids = draw(rows[active], cols[active], t, vocab, slot, seed, call, alias)
        out[active], att[active] = ids, t
        if index is None:
            break
        rej = is_positive(pairs, kpos, vocab, rows[active], ids)
        np.add.at(stats[:, 0], rows[active][rej], 1)
        t += 1
        active = active[rej]
        if t - first_attempt == max_attempts:
            np.add.at(stats[:, 1], rows[active], 1)
            break
    return out.reshape(n, K), stats, att.reshape(n, K)


def build_index(keys, vals, vocab):
    """(sorted unique keys, starts [num_keys + 1], values sorted and unique per key) of (key, value) pairs: the layout of
    kge_amd.eval.FilterIndex."""
    keys, vals = np.asarray(keys, dtype=np.int64), np.asarray(vals, dtype=np.int64)
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    order = np.lexsort((vals, keys))
    k, v = keys[order], vals[order]
    keep = np.ones(len(k), dtype=bool)
    keep[1:] = (k[1:] != k[:-1]) | (v[1:] != v[:-1])
    k, v = k[keep], v[keep]
    uk, start = np.unique(k, return_index=True)
    return uk, np.append(start, len(k)).astype(np.int64), v


def alias_setup(probs):
    """Walker / Vose alias tables of a probability vector: (prob float32 [V], idx int64 [V]) with
    P(id) = (prob[id] + sum_{j: idx[j] = id} (1 - prob[j])) / V."""
    p = np.asarray(probs, dtype=np.float64)
    V = len(p)
    q = p * V / p.sum()
    idx = np.arange(V, dtype=np.int64)
    small = [i for i in range(V) if q[i] < 1.0]
    large = [i for i in range(V) if q[i] >= 1.0]
    while small and large:
        s, l = small.pop(), large[-1]
        idx[s] = l
        q[l] -= 1.0 - q[s]
        if q[l] < 1.0:
            large.pop()
            small.append(l)
    for i in small + large:  # what rounding left over: its own bucket, always
        q[i] = 1.0
    return np.clip(q, 0.0, 1.0).astype(np.float32), idx


def alias_law(prob, idx):
    """The distribution the tables (as stored: float32 prob) draw from, float64."""
    prob = np.asarray(prob, dtype=np.float64)
    V = len(prob)
    law = prob.copy()
    np.add.at(law, idx, 1.0 - prob)
    return law / V
