"""Relational Tucker3 (kge/model/relational_tucker3.py, embedder/tucker3_relation_embedder.py) restated in numpy float64
for the tests (no torch, no GPU): the projection M_p = (B[p] @ W^T).view(d, d), the RESCAL score forms over the projected
matrices, all gradients, and an elementwise float32 rounding bound for each.

The bound follows the rules of tests/_rescal_ref.py (imported, not edited): every quantity is a pair (x, e) with
|fl(x) - x| <= e, u = 2^-24 per written operation, (K - 1) u sum |x_k| for a K-term sum in any order, inputs exact.
The projection is a sum of d_r products of exact inputs; its error e_M then enters every RESCAL form as an INPUT error
on M (the forms of _rescal_ref.py take M exact, so they are restated here with e_M carried).  Backward:

  g_Brows [n, d_r] = g_M [n, d^2] W            a d^2-term sum, g_M with its error
  g_W [d^2, d_r]   = g_M^T B[idx]              an n-term sum
  g_B              = index_add of g_Brows      (c - 1) u sum |x_k| for a row hit c times (_rescal_ref.scatter / accum)

Nothing is tuned or measured.
"""
import numpy as np

import _rescal_ref as rr
from _rescal_ref import U, accum, bound, dot, prod  # noqa: F401


def make_params(E, R, d, dr, seed):
    """float32 entity table, base table B [R, d_r], projection weight W [d^2, d_r]; base row 1 all zero"""
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((E, d)).astype(np.float32)
    B = rng.standard_normal((R, dr)).astype(np.float32)
    W = rng.standard_normal((d * d, dr)).astype(np.float32)
    if R > 1:
        B[1] = 0.0
    return ent, B, W


def project(B, W, idx=None):
    """(M [n, d^2], e): M[i][j] = sum_k B[idx_i][k] W[j][k]"""
    B, W = np.asarray(B, np.float64), np.asarray(W, np.float64)
    rows = B if idx is None else B[np.asarray(idx)]
    return dot(rows[:, None, :], None, W[None, :, :], None)


def _mats(M, eM, d):
    return M.reshape(-1, d, d), eM.reshape(-1, d, d)


def queries(direction, ent, M, eM, a):
    """q [n, d] and its error from per-row matrices M [n, d^2]: "sp_" q = M^T e, "_po" q = M e"""
    e = np.asarray(ent, np.float64)[np.asarray(a)]
    Mm, eMm = _mats(M, eM, e.shape[1])
    if direction == "sp_":
        return dot(e[:, :, None], None, Mm, eMm, axis=1)
    return dot(Mm, eMm, e[:, None, :], None, axis=2)


def score_pairs(direction, ent, M, eM, a, targets=None):
    q, eq = queries(direction, ent, M, eM, a)
    t = np.asarray(ent, np.float64)
    if targets is not None:
        t = t[np.asarray(targets)]
    return dot(q[:, None, :], eq[:, None, :], t[None, :, :], None)


def score_rows(direction, ent, M, eM, a, x):
    q, eq = queries(direction, ent, M, eM, a)
    t = np.asarray(ent, np.float64)[np.asarray(x)]
    if t.ndim == 3:
        return dot(q[:, None, :], eq[:, None, :], t, None)
    return dot(q, eq, t, None)


def score_spo(ent, M, eM, s, o):
    return score_rows("sp_", ent, M, eM, s, o)


def score_neg(ent, M, eM, s, o, slot, neg):
    return score_rows("sp_", ent, M, eM, s, neg) if slot == 2 else score_rows("_po", ent, M, eM, o, neg)


def _row_grads(direction, ent, M, eM, a, gq, egq):
    e = np.asarray(ent, np.float64)[np.asarray(a)]
    n, d = e.shape
    Mm, eMm = _mats(M, eM, d)
    if direction == "sp_":
        ga = dot(Mm, eMm, gq[:, None, :], egq[:, None, :], axis=2)
        gm = prod(e[:, :, None], None, gq[:, None, :], egq[:, None, :])
    else:
        ga = dot(gq[:, :, None], egq[:, :, None], Mm, eMm, axis=1)
        gm = prod(gq[:, :, None], egq[:, :, None], e[:, None, :], None)
    return ga, (gm[0].reshape(n, d * d), gm[1].reshape(n, d * d))


def pairs_bwd(direction, ent, M, eM, a, targets, gout):
    """((g_a, e), (g_M [n, d^2], e), (g_tgt, e)) of sum_ij gout_ij score_ij"""
    g = np.asarray(gout, np.float64)
    t = np.asarray(ent, np.float64)
    if targets is not None:
        t = t[np.asarray(targets)]
    q, eq = queries(direction, ent, M, eM, a)
    gq, egq = dot(g[:, :, None], None, t[None, :, :], None, axis=1)
    gt = dot(g[:, :, None], None, q[:, None, :], eq[:, None, :], axis=0)
    ga, gm = _row_grads(direction, ent, M, eM, a, gq, egq)
    return ga, gm, gt


def rows_bwd(direction, ent, M, eM, a, x, gout):
    """x [n, K] entity ids scored against q(a_i, M_i), gout [n, K]: ((g_a, e), (g_M, e), (g_x [n, K, d], e))"""
    g = np.asarray(gout, np.float64)
    xr = np.asarray(ent, np.float64)[np.asarray(x)]
    q, eq = queries(direction, ent, M, eM, a)
    gq, egq = dot(g[:, :, None], None, xr, None, axis=1)
    gx = prod(g[:, :, None], None, q[:, None, :], eq[:, None, :])
    ga, gm = _row_grads(direction, ent, M, eM, a, gq, egq)
    return ga, gm, gx


def project_bwd(B, W, idx, gM, egM=None):
    """((g_Brows [n, d_r], e), (g_W [d^2, d_r], e)) from g_M [n, d^2] with its error"""
    B, W = np.asarray(B, np.float64), np.asarray(W, np.float64)
    rows = B if idx is None else B[np.asarray(idx)]
    gM = np.asarray(gM, np.float64)
    egM = np.zeros_like(gM) if egM is None else egM
    g_rows = dot(gM[:, :, None], egM[:, :, None], W[None, :, :], None, axis=1)
    g_w = dot(gM[:, :, None], egM[:, :, None], rows[:, None, :], None, axis=0)
    return g_rows, g_w


def base_grad(R, idx, g_rows, e_rows):
    """g_B [R, d_r] = index_add of the row gradients: (sum, error)"""
    if idx is None:
        return g_rows, e_rows
    return accum([(idx, g_rows, e_rows)], (R, g_rows.shape[1]))


def table_grad(R, p, gm, egm):
    """the projected table's gradient [R, d^2] from per-row gradients (route "all"): (sum, error)"""
    return accum([(p, gm, egm)], (R, gm.shape[1]))


def node_grads(ent, B, W, p, route, calls):
    """The parameter gradients ONE autograd node leaves: `calls` = [(kind, s, o, neg, gout), ...] with kind in "sp", "po",
    "spo", "neg0", "neg2", all over the batch's relations p, accumulated into one entity gradient and one relation-row
    gradient (route "all": rows of the projected table; "batch": the batch's own rows), then through ONE projection
    backward.  gout is taken as exact.  ((g_ent, e), (g_B, e), (g_W, e))"""
    ent = np.asarray(ent)
    E, d = ent.shape
    R, n = np.asarray(B).shape[0], len(p)
    if route == "all":
        Ma, eMa = project(B, W)
        M, eM = Ma[p], eMa[p]
    else:
        M, eM = project(B, W, p)
    rel_ids = p if route == "all" else np.arange(n)
    eparts, mparts = [], []
    for kind, s, o, neg, g in calls:
        if kind in ("sp", "po"):
            direction, a = ("sp_", s) if kind == "sp" else ("_po", o)
            ga, gm, gt = pairs_bwd(direction, ent, M, eM, a, None, g)
            eparts += [(np.arange(E), *gt), (a, *ga)]
        else:
            direction, a = ("_po", o) if kind == "neg0" else ("sp_", s)
            x = o[:, None] if kind == "spo" else neg
            ga, gm, gx = rows_bwd(direction, ent, M, eM, a, x, np.asarray(g).reshape(n, -1))
            eparts += [(a, *ga), (x.reshape(-1), gx[0].reshape(-1, d), gx[1].reshape(-1, d))]
        mparts.append((rel_ids, *gm))
    g_ent = accum(eparts, (E, d))
    GM, eGM = accum(mparts, (R if route == "all" else n, d * d))
    if route == "all":
        g_b, g_w = project_bwd(B, W, None, GM, eGM)
    else:
        rows, g_w = project_bwd(B, W, p, GM, eGM)
        g_b = base_grad(R, p, *rows)
    return g_ent, g_b, g_w


def add_nodes(grads):
    """autograd's sum of several nodes' gradients of one parameter, in any order: (sum, error)"""
    val = sum(g[0] for g in grads)
    err = sum(g[1] for g in grads)
    mag = sum(np.abs(g[0]) + g[1] for g in grads)
    return val, err + (len(grads) - 1) * U * mag


def call_scores(ent, B, W, p, kind, s, o, neg):
    """(scores, e) of one recorded call"""
    M, eM = project(B, W, p)
    if kind == "sp":
        return score_pairs("sp_", ent, M, eM, s)
    if kind == "po":
        return score_pairs("_po", ent, M, eM, o)
    if kind == "spo":
        return score_spo(ent, M, eM, s, o)
    return score_neg(ent, M, eM, s, o, 0 if kind == "neg0" else 2, neg)
