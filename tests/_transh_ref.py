"""TransH (kge/model/transh.py:39-78) restated in numpy float64 for the tests (no torch, no GPU): the three score forms,
all gradients, and an elementwise float32 rounding bound for each.

Formulas (relation row = [d_r | w_r], EPS = float32(1e-6) of F.pairwise_distance, w^ = w / max(||w||_2, 1e-12) of
F.normalize, P = I - w^ w^T):

  spo / sp_ / neg (both slots)   v = (P s + d_r) - P o + EPS        score = -||v||_p
  _po                            v = (P o - d_r) - P s + EPS        (the sign differs: EPS lands on the other side)
  u = d score / d v:  L1 -sign(v), sign(0) = 0;  L2 -v / ||v||, 0 where ||v|| = 0;  U = gout * u
  triple form:  g_s = P U,  g_d = U,  g_o = -P U,  g_w^ = (w^.o - w^.s) U + (w^.U) (o - s)
  _po form:     s and o swapped, g_d = -U
  g_w = (g_w^ - (w^.g_w^) w^) / ||w||  where ||w|| >= 1e-12,  else g_w^ / 1e-12

The bound is a running first-order error analysis of the float32 operation sequence of csrc/transh_device.hpp /
transh.hip, carried along the float64 evaluation: every quantity x is a pair (x, e) with |fl(x) - x| <= e, u = 2^-24:

  input                 e = 0
  x +- y                e = e_x + e_y + u |x +- y|                          (no rounding where x or y is an exact zero)
  x * y                 e = |x| e_y + |y| e_x + e_x e_y + u |x y|
  fma(a, b, c)          e = |a| e_b + |b| e_a + e_a e_b + e_c + u |a b + c| (ONE rounding: -ffp-contract=off, fma written;
                                                                             none where a or b is an exact zero)
                        (the products' second-order term is kept: it is all that is left where a value is zero)
  x / y                 e = (e_x + |x / y| e_y) / |y| + u |x / y|           (IEEE division)
  sqrt(x)               e = e_x / (2 sqrt(x)) + u sqrt(x);   sqrt(e_x) where x = 0
  sum of K terms        e = sum e_k + (K - 1) u sum |x_k|                   (ANY order: REDUCE8, wave butterflies, the
                                                                             float atomics of the _accum entry points)
  max(x, c), |x|, -x    e unchanged;   sign(x) is exact where |x| > e_x (the cases are built so: `sign_safe`)

Counted from the device code: ||w||^2 one sum of d fma products; den one sqrt; w^ one division; a(e) one sum of d
products of (w^, e); fixed = fma(-a, w^, e) +- d_r: fma 1 + add 1; v = fma(c, w^, fixed - t) + EPS: sub 1, fma 1, add 1;
L1 sum of d |v|; L2 sum of d squares, sqrt.  Backward (transh.hip, "backward"): u (L2: a division by the recomputed
norm), U = g u, w^.U a sum of d, A / B / C sums over the varying rows, the epilogue's products and sums as written there.
SLACK covers the second-order terms the first-order rules drop.
"""
import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-6))
NORM_EPS = 1e-12
SLACK = 1.0 + 2.0 ** -10
FLOOR = 2.0 ** -126  # a result this small may be flushed or denormal


class T:
    """value + absolute error bound of its float32 evaluation"""

    def __init__(self, x, e=None):
        self.x = np.asarray(x, np.float64)
        self.e = np.zeros_like(self.x) if e is None else np.asarray(e, np.float64)

    def __neg__(self):
        return T(-self.x, self.e)


def _t(x):
    return x if isinstance(x, T) else T(x)


def _zero(a):
    return (a.x == 0) & (a.e == 0)


def add(a, b, sub=False):
    a, b = _t(a), _t(b)
    x = a.x - b.x if sub else a.x + b.x
    exact = _zero(a) | _zero(b)
    return T(x, a.e + b.e + np.where(exact, 0.0, U * np.abs(x)))


def sub(a, b):
    return add(a, b, True)


def mul(a, b):
    a, b = _t(a), _t(b)
    x = a.x * b.x
    return T(x, np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e + U * np.abs(x))


def fma(a, b, c):
    a, b, c = _t(a), _t(b), _t(c)
    x = a.x * b.x + c.x
    exact = _zero(a) | _zero(b)
    return T(x, np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e + c.e + np.where(exact, 0.0, U * np.abs(x)))


def div(a, b):
    a, b = _t(a), _t(b)
    x = a.x / b.x
    return T(x, (a.e + np.abs(x) * b.e) / np.abs(b.x) + U * np.abs(x))


def sqrt(a):
    x = np.sqrt(a.x)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(a.x > 0, a.e / (2 * np.where(x > 0, x, 1.0)) + U * x, np.sqrt(a.e))
    return T(x, e)


def tsum(a, axis, keepdims=False):
    K = a.x.shape[axis]
    return T(a.x.sum(axis, keepdims=keepdims),
             a.e.sum(axis, keepdims=keepdims) + max(K - 1, 0) * U * np.abs(a.x).sum(axis, keepdims=keepdims))


def bound_of(t):
    return SLACK * t.e + FLOOR


# ---- the formulas, on T ------------------------------------------------------------------------------------------------
def _what(W):
    """W [n, d] -> (w^ [n, d], ||w|| [n, 1] as T)"""
    W = _t(W)
    nrm = sqrt(tsum(mul(W, W), 1, keepdims=True))
    den = T(np.maximum(nrm.x, NORM_EPS), nrm.e)
    return div(W, den), nrm


def _fixed(E, Dr, Wh, dsign):
    a = tsum(mul(Wh, E), 1, keepdims=True)
    pe = fma(-a, Wh, E)
    return (add(pe, Dr) if dsign > 0 else sub(pe, Dr)), a


def _v(F, X, Wh, defect, form_po=False):
    """F [n, 1, d], X [n, m, d] (or broadcastable), Wh [n, 1, d] -> v [n, m, d], c [n, m, 1]"""
    c = tsum(mul(Wh, X), 2, keepdims=True)
    v = add(fma(c, Wh, sub(F, X)), EPS)
    if form_po and defect.get("po_eps_wrong_side"):  # EPS as the spo form has it after swapping the roles: -(...) + EPS
        v = add(-fma(c, Wh, sub(F, X)), EPS)
        v = -v
    return v, c


def _score(v, lp):
    if lp == 1.0:
        return -tsum(T(np.abs(v.x), v.e), 2)
    return -sqrt(tsum(mul(v, v), 2))


def _rows(ent, rel, a, p, d):
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    a, p = np.asarray(a).astype(np.int64), np.asarray(p).astype(np.int64)
    return ent[a], rel[p][:, :d], rel[p][:, d:2 * d]


def score_pairs(l_norm, direction, ent, rel, a, p, targets=None, defect=None):
    """kge_score_sp (direction 'sp', a = s) / kge_score_po ('po', a = o): (scores [n, m], bound [n, m])"""
    defect = defect or {}
    ent64 = np.asarray(ent, np.float64)
    d = ent64.shape[1]
    E, Dr, W = _rows(ent, rel, a, p, d)
    X = ent64 if targets is None else ent64[np.asarray(targets).astype(np.int64)]
    Wh, _ = _what(W)
    F, _ = _fixed(E, Dr, Wh, 1 if direction == "sp" else -1)
    Wh3 = T(Wh.x[:, None, :], Wh.e[:, None, :])
    v, _ = _v(T(F.x[:, None, :], F.e[:, None, :]), T(X[None, :, :]), Wh3, defect, direction == "po")
    sc = _score(v, float(l_norm))
    return sc.x, bound_of(sc)


def score_spo(l_norm, ent, rel, s, p, o):
    """kge_score_spo: (scores [n], bound [n]); also one element of kge_score_neg per expanded triple"""
    ent64 = np.asarray(ent, np.float64)
    d = ent64.shape[1]
    E, Dr, W = _rows(ent, rel, s, p, d)
    X = ent64[np.asarray(o).astype(np.int64)]
    Wh, _ = _what(W)
    F, _ = _fixed(E, Dr, Wh, 1)
    v, _ = _v(T(F.x[:, None, :], F.e[:, None, :]), T(X[:, None, :]), T(Wh.x[:, None, :], Wh.e[:, None, :]), {})
    sc = _score(v, float(l_norm))
    return sc.x[:, 0], bound_of(sc)[:, 0]


def score_neg(l_norm, ent, rel, s, p, o, slot, neg):
    """kge_score_neg: (scores [n, K], bound [n, K]) = score_spo on the expanded triples"""
    s, p, o, neg = (np.asarray(x).astype(np.int64) for x in (s, p, o, neg))
    n, K = neg.shape
    tr = [np.repeat(x, K) for x in (s, p, o)]
    tr[slot] = neg.reshape(-1)
    sc, b = score_spo(l_norm, ent, rel, tr[0], tr[1], tr[2])
    return sc.reshape(n, K), b.reshape(n, K)


def _u(v, lp):
    """d score / d v on T [.., d] (reduction over the last axis); sign_safe = every nonzero |v| above its error"""
    if lp == 1.0:
        safe = bool(np.all((np.abs(v.x) > v.e) | ((v.x == 0) & (v.e == 0))))
        return T(-np.sign(v.x)), safe
    nv = sqrt(tsum(mul(v, v), v.x.ndim - 1, keepdims=True))
    zero = nv.x == 0
    safe = bool(np.all(~zero | (nv.e == 0)))
    q = div(v, T(np.where(zero, 1.0, nv.x), nv.e))
    return T(np.where(zero, 0.0, -q.x), np.where(zero, 0.0, q.e)), safe


def _grads(lp, E, Dr, W, X, G, dsign, form, defect):
    """The wave's arithmetic (transh_bwd_rows_kernel): E [n, d] the rows that stay, X [n, K, d] the rows that vary,
    G [n, K].  form 0: v = fma(al_x, w^, fixed(e) - x) + EPS;  form 1 (neg slot 0): v = fma(al_e, w^, fixed(x) - e) + EPS.
    -> g_e [n, d], g_d [n, d], g_w [n, d], g_x [n, K, d] (all T), sign_safe"""
    Wh, nrm = _what(W)
    F, al_e = _fixed(E, Dr, Wh, dsign)
    Wh3 = T(Wh.x[:, None, :], Wh.e[:, None, :])
    E3 = T(np.asarray(E, np.float64)[:, None, :])
    X = _t(X)
    al_x = tsum(mul(Wh3, X), 2, keepdims=True)
    if form == 0:
        v = add(fma(al_x, Wh3, sub(T(F.x[:, None, :], F.e[:, None, :]), X)), EPS)
        if defect.get("po_eps_wrong_side") and dsign < 0:
            v = -add(-fma(al_x, Wh3, sub(T(F.x[:, None, :], F.e[:, None, :]), X)), EPS)
        sg = 1.0
    else:
        Dr3 = T(np.asarray(Dr, np.float64)[:, None, :])
        fx = add(fma(-al_x, Wh3, X), Dr3)
        v = add(fma(T(al_e.x[:, None, :], al_e.e[:, None, :]), Wh3, sub(fx, E3)), EPS)
        sg = -1.0
    u, safe = _u(v, lp)
    Uv = mul(T(np.asarray(G, np.float64)[:, :, None]), u)
    wu = tsum(mul(Wh3, Uv), 2, keepdims=True)
    A = tsum(Uv, 1)
    B = tsum(mul(wu, X), 1)
    C = tsum(mul(al_x, Uv), 1)
    beta = tsum(wu, 1)
    PU = sub(Uv, mul(wu, Wh3))
    g_x = Uv if defect.get("no_P_in_g_x") else PU
    g_x = T(-sg * g_x.x, g_x.e)
    wA = tsum(mul(Wh, A), 1, keepdims=True)
    PA = sub(A, mul(wA, Wh))
    g_e = T(sg * PA.x, PA.e)
    g_d = T((dsign if form == 0 else 1.0) * A.x, A.e)
    gwh = sub(sub(add(C, B), mul(al_e, A)), mul(beta, T(np.asarray(E, np.float64))))
    gwh = T(sg * gwh.x, gwh.e)
    wg = tsum(mul(Wh, gwh), 1, keepdims=True)
    big = nrm.x >= NORM_EPS
    proj = gwh if defect.get("no_normalize_jacobian") else sub(gwh, mul(wg, Wh))
    g1 = div(proj, T(np.where(big, nrm.x, 1.0), nrm.e))
    g0 = div(gwh, NORM_EPS)
    g_w = T(np.where(big, g1.x, g0.x), np.where(big, g1.e, g0.e))
    return g_e, g_d, g_w, g_x, safe


def pairs_bwd(l_norm, direction, ent, rel, a, p, targets, gout, defect=None):
    """kge_score_pairs_bwd: ((g_a [n, d], g_p [n, 2d], g_tgt [m, d]), (bounds ...), sign_safe)"""
    defect = defect or {}
    ent64 = np.asarray(ent, np.float64)
    d = ent64.shape[1]
    E, Dr, W = _rows(ent, rel, a, p, d)
    X = ent64 if targets is None else ent64[np.asarray(targets).astype(np.int64)]
    n = E.shape[0]
    X3 = np.broadcast_to(X[None, :, :], (n,) + X.shape)
    g_e, g_d, g_w, g_x, safe = _grads(float(l_norm), E, Dr, W, X3, gout, 1 if direction == "sp" else -1, 0, defect)
    g_t = tsum(g_x, 0)
    g_p = T(np.hstack([g_d.x, g_w.x]), np.hstack([g_d.e, g_w.e]))
    return (g_e.x, g_p.x, g_t.x), (bound_of(g_e), bound_of(g_p), bound_of(g_t)), safe


def _scatter(table_shape, idx, rows):
    """dense table gradient: the sum of the rows by index (value and bound)"""
    x, e = np.zeros(table_shape), np.zeros(table_shape)
    np.add.at(x, idx, rows.x)
    np.add.at(e, idx, rows.e)
    cnt = np.zeros(table_shape[0])
    np.add.at(cnt, idx, 1.0)
    mag = np.zeros(table_shape)
    np.add.at(mag, idx, np.abs(rows.x))
    return x, e, cnt, mag


def neg_bwd_accum(l_norm, ent, rel, s, p, o, slot, neg, gout):
    """kge_score_neg_bwd_accum (and, with neg = o[:, None], slot 2, kge_score_spo_bwd_accum) on zeroed gradients:
    ((grad_ent [E, d], grad_rel [R, 2d]), (bounds), sign_safe).  The atomics add the terms of a table row in any order:
    (terms - 1) u sum |term| on top of the terms' own bounds."""
    ent64, rel64 = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    d = ent64.shape[1]
    s, p, o, neg = (np.asarray(x).astype(np.int64) for x in (s, p, o, neg))
    e_idx = o if slot == 0 else s
    E, Dr, W = _rows(ent, rel, e_idx, p, d)
    g_e, g_d, g_w, g_x, safe = _grads(float(l_norm), E, Dr, W, ent64[neg], gout, 1, 1 if slot == 0 else 0, {})
    n, K = neg.shape
    rows = T(np.concatenate([g_e.x, g_x.x.reshape(n * K, d)]), np.concatenate([g_e.e, g_x.e.reshape(n * K, d)]))
    idx = np.concatenate([e_idx, neg.reshape(-1)])
    ge, ge_e, cnt, mag = _scatter(ent64.shape, idx, rows)
    ge_e = ge_e + np.maximum(cnt - 1, 0)[:, None] * U * mag
    g_p = T(np.hstack([g_d.x, g_w.x]), np.hstack([g_d.e, g_w.e]))
    gr, gr_e, cnt, mag = _scatter(rel64.shape, p, g_p)
    gr_e = gr_e + np.maximum(cnt - 1, 0)[:, None] * U * mag
    return (ge, gr), (SLACK * ge_e + FLOOR, SLACK * gr_e + FLOOR), safe


def spo_bwd(l_norm, ent, rel, s, p, o, gout):
    """kge_score_spo_bwd: ((g_s [n, d], g_p [n, 2d], g_o [n, d]), (bounds), sign_safe)"""
    ent64 = np.asarray(ent, np.float64)
    d = ent64.shape[1]
    E, Dr, W = _rows(ent, rel, s, p, d)
    X = ent64[np.asarray(o).astype(np.int64)][:, None, :]
    g_e, g_d, g_w, g_x, safe = _grads(float(l_norm), E, Dr, W, X, np.asarray(gout, np.float64)[:, None], 1, 0, {})
    g_p = T(np.hstack([g_d.x, g_w.x]), np.hstack([g_d.e, g_w.e]))
    g_o = T(g_x.x[:, 0], g_x.e[:, 0])
    return (g_e.x, g_p.x, g_o.x), (bound_of(g_e), bound_of(g_p), bound_of(g_o)), safe


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------
def make_tables(E, R, d, seed, zero_w_row=True, zero_pair=True):
    """float32 tables.  Relation 0 has w = 0 (w^ = 0: the plain TransE distance); with zero_pair, entity 0 is the zero row
    and relation 1 is d_r = -EPS, w = 0: the triple (0, 1, 0) has v = 0 exactly (the zero-distance pair of L2)."""
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((E, d)).astype(np.float32)
    rel = rng.standard_normal((R, 2 * d)).astype(np.float32)
    if zero_w_row:
        rel[0, d:] = 0.0
    if zero_pair and R > 1:
        ent[0] = 0.0
        rel[1, :d] = -np.float32(1e-6)
        rel[1, d:] = 0.0
    return ent, rel
