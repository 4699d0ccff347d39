"""RESCAL (kge/model/rescal.py:14-52) restated in numpy float64 for the tests (no torch, no GPU): the score forms, all
gradients, and an elementwise float32 rounding bound for each.

Formulas (relation row = M, row-major d x d):

  sp_ / spo / neg slot 2     q = M^T s,   score = q . o
  _po / neg slot 0           q = M o,     score = q . s
  backward, g_q = sum_j gout_j x_j over the rows x_j scored against q,  g_x_j = gout_j q:
    sp_ form   g_s = M g_q,    g_M[a][b] = s_a g_q_b
    _po form   g_o = M^T g_q,  g_M[a][b] = g_q_a o_b

The bound follows the rules of tests/_transh_ref.py's docstring, carried along the float64 evaluation: every quantity x
is a pair (x, e) with |fl(x) - x| <= e, u = 2^-24 per written operation, inputs exact.  Everything here is a sum of K
products (csrc/rescal_device.hpp, the float32 chains of DESIGN.md section 4, the gradient products of bwd_gemm32.hip, the
float atomics of the _accum entries), for which the rules give, in ANY summation order and with or without fused
multiply-adds:

  sum_k a_k b_k    e = sum_k (|a_k| e_b + |b_k| e_a + e_a e_b)            the input errors through the partials
                     + K u sum_k (|a_k| + e_a)(|b_k| + e_b)               u per product + (K - 1) u sum |x_k| for the sum,
                                                                          taken on the largest values the float32 terms
                                                                          can have (the second-order terms kept)
  a * b            the same with K = 1

SLACK covers the terms of order u^2 K^2 that a first-order (K - 1) u rule drops; FLOOR a result that is flushed or
denormal.  Nothing is tuned or measured.
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
FLOOR = 2.0 ** -126


def dot(a, ea, b, eb, axis=-1, K=None):
    """(value, error) of sum_k a_k b_k over `axis` (a, b broadcast against each other)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ea = np.zeros_like(a) if ea is None else ea
    eb = np.zeros_like(b) if eb is None else eb
    x = (a * b).sum(axis)
    K = (a * b).shape[axis] if K is None else K
    e = (np.abs(a) * eb + np.abs(b) * ea + ea * eb).sum(axis) + K * U * ((np.abs(a) + ea) * (np.abs(b) + eb)).sum(axis)
    return x, e


def prod(a, ea, b, eb):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ea = np.zeros_like(a) if ea is None else ea
    eb = np.zeros_like(b) if eb is None else eb
    return a * b, np.abs(a) * eb + np.abs(b) * ea + ea * eb + U * (np.abs(a) + ea) * (np.abs(b) + eb)


def bound(e):
    return SLACK * e + FLOOR


def make_tables(E, R, d, seed):
    """float32 tables; non-symmetric M (a transposed matrix is visible), relation 1 all zero, relation 2 the identity"""
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((E, d)).astype(np.float32)
    rel = rng.standard_normal((R, d, d)).astype(np.float32)
    rel += np.triu(np.ones((d, d), np.float32), 1) * 0.75  # a systematic asymmetry on top of the random one
    if R > 1:
        rel[1] = 0.0
    if R > 2:
        rel[2] = np.eye(d, dtype=np.float32)
    return ent, rel.reshape(R, d * d)


def _mats(rel, p, d):
    return np.asarray(rel, np.float64)[np.asarray(p)].reshape(-1, d, d)


def queries(direction, ent, rel, a, p):
    """q [n, d] and its error: "sp_" q = M^T e, "_po" q = M e"""
    e = np.asarray(ent, np.float64)[np.asarray(a)]
    d = e.shape[1]
    M = _mats(rel, p, d)
    if direction == "sp_":
        return dot(e[:, :, None], None, M, None, axis=1)  # sum over a: e_a M[a][b]
    return dot(M, None, e[:, None, :], None, axis=2)      # sum over b: M[a][b] e_b


def score_pairs(direction, ent, rel, a, p, targets=None):
    q, eq = queries(direction, ent, rel, a, p)
    t = np.asarray(ent, np.float64)
    if targets is not None:
        t = t[np.asarray(targets)]
    return dot(q[:, None, :], eq[:, None, :], t[None, :, :], None)


def score_rows(direction, ent, rel, a, p, x):
    """score of q(a_i, p_i) against entity x_i (x [n]) or x_ik (x [n, K])"""
    q, eq = queries(direction, ent, rel, a, p)
    t = np.asarray(ent, np.float64)[np.asarray(x)]
    if t.ndim == 3:
        return dot(q[:, None, :], eq[:, None, :], t, None)
    return dot(q, eq, t, None)


def score_spo(ent, rel, s, p, o):
    return score_rows("sp_", ent, rel, s, p, o)


def score_neg(ent, rel, s, p, o, slot, neg):
    return score_rows("sp_", ent, rel, s, p, neg) if slot == 2 else score_rows("_po", ent, rel, o, p, neg)


def _row_grads(direction, ent, rel, a, p, gq, egq):
    """(g_a, e), (g_M [n, d*d], e) from g_q"""
    e = np.asarray(ent, np.float64)[np.asarray(a)]
    n, d = e.shape
    M = _mats(rel, p, d)
    if direction == "sp_":
        ga = dot(M, None, gq[:, None, :], egq[:, None, :], axis=2)   # M g_q
        gm = prod(e[:, :, None], None, gq[:, None, :], egq[:, None, :])
    else:
        ga = dot(gq[:, :, None], egq[:, :, None], M, None, axis=1)   # M^T g_q
        gm = prod(gq[:, :, None], egq[:, :, None], e[:, None, :], None)
    return ga, (gm[0].reshape(n, d * d), gm[1].reshape(n, d * d))


def pairs_bwd(direction, ent, rel, a, p, targets, gout):
    """((g_a, e), (g_p, e), (g_tgt, e)) of sum_ij gout_ij score_ij"""
    g = np.asarray(gout, np.float64)
    t = np.asarray(ent, np.float64)
    if targets is not None:
        t = t[np.asarray(targets)]
    q, eq = queries(direction, ent, rel, a, p)
    gq, egq = dot(g[:, :, None], None, t[None, :, :], None, axis=1)          # [n, d]: sum over the targets
    gt = dot(g[:, :, None], None, q[:, None, :], eq[:, None, :], axis=0)     # [m, d]: sum over the queries
    ga, gm = _row_grads(direction, ent, rel, a, p, gq, egq)
    return ga, gm, gt


def rows_bwd(direction, ent, rel, a, p, x, gout):
    """x [n, K] entity ids scored against q(a_i, p_i), gout [n, K]: ((g_a, e), (g_p, e), (g_x [n, K, d], e))"""
    g = np.asarray(gout, np.float64)
    xr = np.asarray(ent, np.float64)[np.asarray(x)]
    q, eq = queries(direction, ent, rel, a, p)
    gq, egq = dot(g[:, :, None], None, xr, None, axis=1)
    gx = prod(g[:, :, None], None, q[:, None, :], eq[:, None, :])
    ga, gm = _row_grads(direction, ent, rel, a, p, gq, egq)
    return ga, gm, gx


def scatter(shape, ids, val, err):
    """per-row results added into a table in float64: (sum, bound of the float32 atomics' sum in any order).  A sum of c
    terms adds (c - 1) u sum |x_k|, taken on the largest values the float32 terms can have."""
    ids = np.asarray(ids).reshape(-1)
    val, err = val.reshape(len(ids), -1), err.reshape(len(ids), -1)
    out, e, ab = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    cnt = np.zeros(shape[0])
    np.add.at(out, ids, val)
    np.add.at(e, ids, err)
    np.add.at(ab, ids, np.abs(val) + err)
    np.add.at(cnt, ids, 1.0)
    return out, e, ab, cnt


def accum(parts, shape):
    """parts: [(ids, val, err), ...] all added into one [rows, width] table: (sum, error)"""
    out, e, ab, cnt = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape[0])
    for ids, val, err in parts:
        o2, e2, a2, c2 = scatter(shape, ids, val, err)
        out, e, ab, cnt = out + o2, e + e2, ab + a2, cnt + c2
    return out, e + np.maximum(cnt - 1, 0)[:, None] * U * ab
