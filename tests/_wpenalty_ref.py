"""numpy restatements of the frequency-weighted penalty terms (kge_amd/csrc/wpenalty.hip).

truth():  float64, from the reference's formula as lookup_embedder.py:148-173 writes it -- unique / counts /
          len(indexes).  len() of the [n, 2] block kge_model.py:616-618 builds for a shared entity embedder is n: its 2n
          entries are divided by n.
The rest: float32, operation for operation what the four kernels do per element, in the style of _optim_ref.py and
          _sparse_adam_ref.py (whose updates they reuse): the row factor f_r = weight * (float32(c_r) / float32(m)) --
          one division, then one product --, the term's gradient under f_r, added to the gradient of the rows whose
          count is not 0 only.
"""
import numpy as np

import _adam_multi_ref as amr
import _optim_ref as orf
import _sparse_adam_ref as sar
from _touched_ref import marked_rows

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def counts_of(ids, num_rows):
    """What kge_penalty_count leaves: occurrences per row, ids outside [0, num_rows) dropped."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    ids = ids[(ids >= 0) & (ids < num_rows)]
    return np.bincount(ids, minlength=num_rows).astype(np.uint32)


def _norms64(x, kind):
    x = np.asarray(x, dtype=np.float64)
    if kind == "n3_complex":
        h = x.shape[1] // 2
        return np.sqrt(x[:, :h] ** 2 + x[:, h:] ** 2 + 1e-14)
    return np.abs(x)


def truth(table, indexes, kind, p, weight):
    """float64 (value, gradient [V, d]) of the weighted term: `indexes` as the embedder gets them (1-D, or [n, 2])."""
    table = np.asarray(table, dtype=np.float64)
    indexes = np.asarray(indexes)
    uniq, counts = np.unique(indexes, return_counts=True)
    m = len(indexes)
    p = 3 if kind == "n3_complex" else p
    rows = table[uniq]
    a = _norms64(rows, kind)
    value = (weight / p * (a ** p * counts.astype(np.float64).reshape(-1, 1))).sum() / m
    grad = np.zeros_like(table)
    fac = weight * counts.astype(np.float64).reshape(-1, 1) / m
    if kind == "n3_complex":
        grad[uniq] = fac * np.concatenate([a * a, a * a], axis=1) / np.concatenate([a, a], axis=1) * rows  # |z| * x
    else:
        grad[uniq] = fac * np.sign(rows) * a ** (p - 1)
    return value, grad


def value_sum64(table, counts, kind, p):
    """sum_r c_r sum_j |x_rj|^p in float64: what *value holds, exactly."""
    a = _norms64(table, kind)
    p = 3 if kind == "n3_complex" else p
    return float((a ** p * np.asarray(counts, dtype=np.float64).reshape(-1, 1)).sum())


def value_bound(table, counts, kind, p, workgroups):
    """|device value - value_sum64| <= this.  Per element the kernel forms t = |x|^p in float32 (lp: p - 1 products;
    n3: two squares, two sums, a square root, two products -- relative error below 10 u),
    multiplies by the count in float64 (exact) and adds in float64: every partial sum below the total S of the
    non-negative terms, at most (elements per thread + 6 + 4 + workgroups) additions deep."""
    k = 10 if kind == "n3_complex" else (p - 1)
    s = value_sum64(table, counts, kind, p)
    depth = np.asarray(table).shape[1] + 16 + workgroups
    rel = k * U32 / (1 - k * U32) + depth * U64
    if kind == "n3_complex":  # the float32 constant 1e-14f is not 1e-14: |z|^3 moves by at most 1.5 |z| * 2^-24 * 1e-14
        rel += 1e-20
    return s * rel + 1e-300


def factors(counts, m, weight):
    """float32 f_r and the mask of rows that take the term."""
    c = np.asarray(counts, dtype=np.uint32)
    with np.errstate(**orf._QUIET):
        f = np.float32(weight) * (c.astype(np.float32) / np.float32(m))
    return f.astype(np.float32), c != 0


def penalty_gradient(table, counts, m, kind, p, weight):
    """float32 [V, d] gradient of the term under the row factors, and the [V] mask of rows it is added to."""
    x = np.array(table, dtype=np.float32)
    f, add = factors(counts, m, weight)
    f = f.reshape(-1, 1)
    with np.errstate(**orf._QUIET):
        if kind == "n3_complex":
            h = x.shape[1] // 2
            re, im = x[:, :h], x[:, h:]
            z = np.sqrt(re * re + im * im + np.float32(1e-14))
            pg = np.concatenate([f * (z * re), f * (z * im)], axis=1)
        elif p == 1:
            pg = np.where(x > 0, f, np.where(x < 0, -f, np.float32(0)))
        elif p == 2:
            pg = f * x
        elif p == 3:
            pg = f * (x * np.abs(x))
        else:
            raise ValueError(p)
    return pg.astype(np.float32), add


def _with_term(grad, pg, add):
    g = np.array(grad, dtype=np.float32)
    with np.errstate(**orf._QUIET):
        return np.where(add.reshape(-1, 1), g + pg, g).astype(np.float32)


def adagrad_dense(param, grad, sum, counts, m, kind, p, weight, minus_clr, weight_decay, eps):
    """kge_adagrad_step_multi_wpenalty on one [V, d] table -> (param, sum, bf16 bits)."""
    pg, add = penalty_gradient(param, counts, m, kind, p, weight)
    pn, sn = orf.adagrad(param, _with_term(grad, pg, add), sum, minus_clr, weight_decay, eps)
    shape = np.asarray(param).shape
    return pn.reshape(shape), sn.reshape(shape), orf.bf16_rne_bits(pn).reshape(shape)


def adam_dense(param, grad, m1, m2, clock, lr, beta1, beta2, counts, m, kind, p, weight, weight_decay, eps):
    """kge_adam_step_multi_wpenalty on one [V, d] table -> (param, m1, m2, bf16 bits, clock)."""
    clock = amr.clock_tick(clock, lr, beta1, beta2)
    pg, add = penalty_gradient(param, counts, m, kind, p, weight)
    pn, a, b = orf.adam(param, _with_term(grad, pg, add), m1, m2, clock[3], clock[4], beta1, beta2, weight_decay, eps)
    shape = np.asarray(param).shape
    return pn.reshape(shape), a.reshape(shape), b.reshape(shape), orf.bf16_rne_bits(pn).reshape(shape), clock


def adagrad_touched(param, grad, sum, bitmap, counts, m, kind, p, weight, minus_clr, eps, copy=None):
    """kge_adagrad_step_touched_wpenalty -> (param, grad, sum, copy) after it: marked rows only."""
    pn, gn, sn = (np.array(x, dtype=np.float32) for x in (param, grad, sum))
    cn = None if copy is None else np.array(copy, dtype=np.uint16)
    pg, add = penalty_gradient(param, counts, m, kind, p, weight)
    g = _with_term(grad, pg, add)
    for r in marked_rows(bitmap, pn.shape[0]):
        pr, sr = orf.adagrad(pn[r], g[r], sn[r], minus_clr, 0.0, eps)
        pn[r], sn[r], gn[r] = pr, sr, 0
        if cn is not None:
            cn[r] = orf.bf16_rne_bits(pr)
    return pn, gn, sn, cn


def sparse_adam_touched(param, grad, m1, m2, bitmap, clock, lr, beta1, beta2, counts, m, kind, p, weight, eps,
                        copy=None):
    """kge_sparse_adam_step_touched_wpenalty -> (param, grad, m1, m2, copy, clock) after it."""
    pg, add = penalty_gradient(param, counts, m, kind, p, weight)
    g = _with_term(grad, pg, add)
    pn, gn, a, b, _bm, cn, clock = sar.step_touched(param, g, m1, m2, bitmap, clock, lr, beta1, beta2, eps, copy)
    return pn, gn, a, b, cn, clock
