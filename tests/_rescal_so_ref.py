"""RESCAL relation prediction (csrc/rescal_so.hip) restated in numpy float64: the [n, m] scores s_i^T M_{r_j} o_i, the
three gradients of sum_ij g_ij score_ij, and a float32 bound for each, derived with the rules of tests/_rescal_ref.py
(u = 2^-24 per written operation, K u sum |terms| for a sum of K products in any order, fused or not).

  scores    A_i[a, b] = fl(s_a o_b): one u.  score = sum over K = d^2 of A M.  The MFMA chain, the zero padding and the
            K splits' ordered adds are one summation order of those d^2 terms: (d^2 + 1) u sum |s_a M_ab o_b|.
  grad_rel  per entry j of rels: sum over K = n pairs of g_ij A_i; the entries that name one relation and the pre-filled
            value are added one by one (plain or atomic): accum().
  grad_ent  per tile of TJ relations (the kernel's tile): W = sum over K = |tile| of g_ij M_j, then g_s = W o and
            g_o = s^T W over K = d; the tiles' rows and the pre-filled value are added by atomics: accum().
Nothing is tuned or measured."""
import numpy as np

from _rescal_ref import U, accum, dot

TJ = 32  # RSO_TJ: relations per workgroup of rso_entgrad_kernel


def _outer(ent, s, o):
    e = np.asarray(ent, np.float64)
    A = (e[s][:, :, None] * e[o][:, None, :]).reshape(len(s), -1)
    return A, U * np.abs(A)


def scores(ent, rel, s, o, rels):
    """(scores [n, m], error)"""
    A, eA = _outer(ent, s, o)
    M = np.asarray(rel, np.float64)[rels]
    return dot(A[:, None, :], eA[:, None, :], M[None], None)


def grads(ent, rel, s, o, rels, g, ge0, gr0):
    """((grad_ent, error), (grad_rel, error)) after accumulating into the float32 pre-fills ge0, gr0"""
    e = np.asarray(ent, np.float64)
    g = np.asarray(g, np.float64)
    n, d = len(s), e.shape[1]
    A, eA = _outer(ent, s, o)
    M = np.asarray(rel, np.float64)[rels]
    val, err = dot(g[:, :, None], None, A[:, None, :], eA[:, None, :], axis=0)  # [m, d^2], K = n
    zr = np.zeros_like(gr0, np.float64)
    g_rel = accum([(rels, val, err), (np.arange(len(gr0)), gr0.astype(np.float64), zr)], gr0.shape)
    ze = np.zeros_like(ge0, np.float64)
    parts = [(np.arange(len(ge0)), ge0.astype(np.float64), ze)]
    for j0 in range(0, len(rels), TJ):
        W, eW = dot(g[:, j0:j0 + TJ, None], None, M[None, j0:j0 + TJ], None, axis=1)  # [n, d^2]
        W, eW = W.reshape(n, d, d), eW.reshape(n, d, d)
        parts.append((s,) + dot(W, eW, e[o][:, None, :], None, axis=2))   # g_s[a] = W[a, :] . o
        parts.append((o,) + dot(e[s][:, :, None], None, W, eW, axis=1))   # g_o[b] = sum_a s_a W[a, b]
    return accum(parts, ge0.shape), g_rel
