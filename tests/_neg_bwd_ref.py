"""The triple-wise backward entry points of bwd.hip restated in numpy float64 for the tests (no torch, no GPU), with an
elementwise rounding bound: kge_score_spo_bwd, kge_score_spo_bwd_accum, kge_score_neg_bwd_accum and
kge_score_neg_bwd_accum_sorted (the last two compute the same sums).

  spo_bwd(name, l_norm, ent, rel, s, p, o, gout) -> (g_s [n, d], g_p [n, d_r], g_o [n, d]) per triple
  spo_bwd_accum(..., ge0, gr0)                   -> (grad_ent [E, d], grad_rel [R, d_r]): the rows scatter-added on top
                                                    of the given initial contents
  neg_bwd_accum(..., slot, neg, gout, ge0, gr0)  -> the same for triple i with `slot` replaced by neg[i, k]: it IS
                                                    spo_bwd_accum on the n K expanded triples, and is computed so

The row gradients are the closed forms of spo_pair_grads (bwd_device.hpp) from the scorer definitions
(oracle/torch_port.py score_emb, combine "spo"), per coordinate pair (x0 = first half, x1 = second half):

  distmult  ds = g r o, dp = g s o, do = g s r
  complex   ds0 = g (o0 r0 + o1 r1), ds1 = g (o1 r0 - o0 r1);  dp0 = g (o0 s0 + o1 s1), dp1 = g (o1 s0 - o0 s1);
            do0 = g (s0 r0 - s1 r1), do1 = g (s1 r0 + s0 r1)
  transe    e = s + r - o + 1e-6 (F.pairwise_distance adds its eps to EVERY component: an exact tie weighs
            sign(+1e-6) = +1 under l_norm 1, where the pair path -- torch.cdist, no eps -- has 0), score = -||e||_p,
            w = sign(e) (|e| / dist)^(p-1):  ds = dp = -g w, do = g w
  rotate    q = s e^{i r}, score = -|| |q - o| ||_p, w = (q - o) |q - o|^(p-2) / dist^(p-1), dq = -g w:
            ds = dq e^{-i r} (ds0 = dq0 c + dq1 s, ds1 = dq1 c - dq0 s), dp = dq1 q0 - dq0 q1, do = -dq

The weights come from _pairs_bwd_ref (_transe_w, _rotate_w, _pnorm_w: the device functions transe_w / rotate_w are the
pair path's), called with the difference s + r - o (q - o) as the "query" against the origin as the one "target".

Bound, elementwise: |float32 result - reference| <= (K_e + C) u A_e, u = 2^-24, the rules of _pairs_bwd_ref:
  K_e  the number of terms this call adds into the table element (occurrences of the row as s, o and corrupted entity,
       or of the relation as p), plus 1 where the table was pre-loaded.  (K - 1) u bounds a float32 sum of K terms in
       ANY order: register partials over a chunk, a chunk's flush, float atomics, the sorted kernel's runs.  An element
       no term goes to keeps its bits: bound 0.
  A_e  the same sums on magnitudes (every subtraction an addition, cos and sin 1, a divisor with its true value and its
       condition number), plus |initial content|.
  C    the float32 roundings of one term on its longest path, c_counts() below: from spo_pair_grads, transe_w,
       rotate_w and, for l_norm != 1, the stored forward score that supplies `dist` (spo_device.hpp apply_chunk /
       finalize, the same arithmetic in kge_score_spo and in both slots of kge_score_neg).  ROTPRE reads the same
       sincos_canon values from rot_table_kernel's table.

The fixed case lists of tests/test_gpu_neg_bwd.py are built here (NEG_CASES, SPO_CASES, ACC_CASES, make_case), so that
tests/test_neg_bwd_ref_cpu.py checks the very inputs the GPU file runs; neg_chunk / spo_chunk / sorted_nc restate the
host launch rules of bwd.hip and `branches` evaluates them per case.
"""
import math

import numpy as np

from _pairs_bwd_ref import C_CHAIN_A, C_CHAIN_P, C_POW, C_Q, U, _c_weight, _mag, _pnorm_w, _rotate_w, _transe_w

EPS = 1e-6
C_E_TRANSE = 3  # e = ((s + r) - o) + 1e-6f: three sums (the constant's own rounding is below u of the sum's scale)


# ---- the counts --------------------------------------------------------------------------------------------------------
def c_weight(name, lp, d):
    """roundings on the path to the weight w of one term (0 for the dot-product scorers)"""
    if name in ("complex", "distmult"):
        return 0
    if name == "transe":
        c_e = C_E_TRANSE
        if lp == 1.0:
            return c_e  # sign(e): exact once the sign is right (grid inputs)
        if lp == 2.0:  # stored score: d fused squares and a root, (c_e + d / 2 + 1) u S_dist;  w = e / dist: + 1
            return max(c_e, c_e + math.ceil(d / 2) + 1) + 1
        # dist = powf(sum powf(|e|, p), 1 / p): (c_e + (d + 2) / p + 4) u S_dist;  w = powf(|e|, p-1) / powf(dist, p-1)
        c_dist = c_e + math.ceil((d + 2) / lp) + 4
        return math.ceil((lp - 1) * max(c_e, c_dist)) + 2 * C_POW + 1
    if lp in (1.0, 2.0):
        return _c_weight("rotate", lp, d)  # the pair path's count: the same q, q - o, modulus, distance, f, e f
    h = d // 2
    c_e = C_Q["rotate"] + 1
    c_ab = c_e + 2
    c_dist = c_ab + math.ceil((h + 2) / lp) + 4  # powf per modulus, h sums, powf(., 1 / p) with 1 / p rounded
    # f = powf(ab, p-2) / powf(dist, p-1): the powers multiply the operands' relative errors, two powf, the division
    c_f = max(math.ceil((lp - 2) * c_ab), math.ceil((lp - 1) * c_dist)) + C_POW + 1
    return max(c_e, c_f) + 1  # w = e f


def c_counts(name, l_norm, d):
    """(C of an s-row term, of a p-row term, of an o-row term) of spo_pair_grads:
      distmult  g * (x * y): 2                      complex  g * (x y +- x' y'): product 1, sum 1, g: 3
      transe    -g * w: c_weight + 1 (ds = dp = -do: exact copies)
      rotate    dq = -g * w: c_weight + 1;  ds = dq c +- dq' s: + sincos 2 + product 1 + sum 1;  dp = dq' q - dq q':
                + query 4 + product 1 + sum 1;  do = -dq: + 0"""
    if name == "distmult":
        return 2, 2, 2
    if name == "complex":
        return 3, 3, 3
    cw = c_weight(name, float(l_norm), d) + 1
    if name == "transe":
        return cw, cw, cw
    return cw + C_CHAIN_A["rotate"], cw + C_CHAIN_P["rotate"], cw


# ---- row gradients of N triples ------------------------------------------------------------------------------------------
def _halves(X):
    h = X.shape[1] // 2
    return X[:, :h], X[:, h:]


def _row_grads(name, lp, S, R, O, g, eps, flip, want_bound, min_ab=None):
    """S, O [N, d], R [N, d_r] gathered rows, g [N] -> (gs, gp, go), their companions (or None)"""
    g = g[:, None]
    ag = np.abs(g)
    comp = None
    if name == "distmult":
        val = (g * R * O, g * S * O, g * S * R)
        if want_bound:
            aS, aR, aO = np.abs(S), np.abs(R), np.abs(O)
            comp = (ag * aR * aO, ag * aS * aO, ag * aS * aR)
        return val, comp
    if name == "complex":
        def forms(s0, s1, r0, r1, o0, o1, w, sg, f):
            return (np.hstack([w * (o0 * r0 + o1 * r1), w * (o1 * r0 + f * o0 * r1)]),
                    np.hstack([w * (o0 * s0 + o1 * s1), w * (o1 * s0 + sg * o0 * s1)]),
                    np.hstack([w * (s0 * r0 + sg * s1 * r1), w * (s1 * r0 + s0 * r1)]))
        val = forms(*_halves(S), *_halves(R), *_halves(O), g, -1.0, 1.0 if flip else -1.0)
        if want_bound:
            comp = forms(*_halves(np.abs(S)), *_halves(np.abs(R)), *_halves(np.abs(O)), ag, 1.0, 1.0)
        return val, comp
    origin = np.zeros((1, S.shape[1]))
    if name == "transe":
        W, SW = _transe_w(S + R - O, np.abs(S) + np.abs(R) + np.abs(O) + eps, origin, lp, eps)
        W, SW = W[:, 0, :], SW[:, 0, :]
        return (-g * W, -g * W, g * W), ((ag * SW,) * 3 if want_bound else None)
    (s0, s1), (o0, o1), cs, sn = _halves(S), _halves(O), np.cos(R), np.sin(R)
    q0, q1 = s0 * cs - s1 * sn, s0 * sn + s1 * cs
    Sqs = np.abs(s0) + np.abs(s1)
    Sq = Sqs + np.maximum(np.abs(o0), np.abs(o1))  # one scale for both components of q - o
    wre, wim, swre, swim, ab = _rotate_w(q0 - o0, q1 - o1, Sq, origin, lp)
    if min_ab is not None and ab.size:
        min_ab.append(float(ab.min()))
    if want_bound and lp not in (1.0, 2.0):
        # w = e ab^(p-2) / dist^(p-1): the condition numbers of the modulus and of the distance, their exponents in C
        ab3 = ab
        Se = Sq[:, None, :]
        Sab = 2.0 * Se ** 2 / ab3
        dist, Sd, _ = _pnorm_w(ab3, Sab, lp)
        f = ab3 ** (lp - 2.0) / dist ** (lp - 1.0)
        kap = Sab / ab3 + Sd / dist
        swre, swim = Se * f + np.abs(wre) * kap, Se * f + np.abs(wim) * kap
    wre, wim = wre[:, 0, :], wim[:, 0, :]
    dq0, dq1 = -g * wre, -g * wim
    val = (np.hstack([dq0 * cs + dq1 * sn, dq1 * cs - dq0 * sn]), dq1 * q0 - dq0 * q1, np.hstack([-dq0, -dq1]))
    if want_bound:
        a0, a1 = ag * swre[:, 0, :], ag * swim[:, 0, :]
        comp = (np.hstack([a0 + a1, a0 + a1]), (a0 + a1) * Sqs, np.hstack([a0, a1]))
    return val, comp


def _zero_last(name, X):
    """the last coordinate (pair) of the rows read as zero"""
    X = X.copy()
    d = X.shape[1]
    X[:, d - 1] = 0.0
    if name in ("complex", "rotate"):
        X[:, d // 2 - 1] = 0.0
    return X


def _gather(name, ent, rel, S, P, O, defect, dtype=np.float64):
    ent, rel = np.asarray(ent, dtype), np.asarray(rel, dtype)
    S, P, O = (np.asarray(x).astype(np.int64) for x in (S, P, O))
    Sr, Rr, Or = ent[S], rel[P], ent[O]
    side = defect.get("zero_last")
    if side == "s":
        Sr = _zero_last(name, Sr)
    if side == "o":
        Or = _zero_last(name, Or)
    return Sr, Rr, Or


def _scatter(tab, idx, rows):
    """tab[idx[j], :] += rows[j, :]"""
    if rows.shape[0] > 4096 and rows.shape[1] <= 8:
        for c in range(rows.shape[1]):
            tab[:, c] += np.bincount(idx, weights=rows[:, c], minlength=tab.shape[0])
    else:
        np.add.at(tab, idx, rows)


def _accum(name, l_norm, ent, rel, S, P, O, g, ge0, gr0, defect, want_bound, min_ab=None):
    """spo_bwd_accum on N triples -> (grad_ent, grad_rel), (bound_ent, bound_rel) or None.  Planted defects:
      drop = (dests, js)    the contributions of triples js to the destinations in dests ("s", "p", "o") left out
      move = (dest, j, e)   triple j's `dest` contribution credited to row e
      rel_next = shift, zero_last = "s" / "o", flip_cross, eps, overwrite"""
    defect = defect or {}
    lp = float(l_norm)
    S, P, O = (np.asarray(x).astype(np.int64).copy() for x in (S, P, O))
    g = np.asarray(g, np.float64).reshape(-1)
    # row i + 1's relation row read for row i (rel_next = the triples per row: K in an expanded call, else 1)
    Pg = np.roll(P, -int(defect["rel_next"])) if defect.get("rel_next") else P
    Sr, Rr, Or = _gather(name, ent, rel, S, Pg, O, defect)
    val, comp = _row_grads(name, lp, Sr, Rr, Or, g, float(defect.get("eps", EPS)), bool(defect.get("flip_cross")),
                           want_bound, min_ab)
    val = [v.copy() for v in val]
    if defect.get("drop"):
        dests, js = defect["drop"]
        for k, key in enumerate("spo"):
            if key in dests:
                val[k][np.asarray(js)] = 0.0
    dest = {"s": S, "p": P, "o": O}
    if defect.get("move"):
        key, j, e = defect["move"]
        dest[key][j] = e
    ge0, gr0 = np.asarray(ge0, np.float64), np.asarray(gr0, np.float64)
    te, tr = np.zeros_like(ge0), np.zeros_like(gr0)
    _scatter(te, dest["s"], val[0])
    _scatter(te, dest["o"], val[2])
    _scatter(tr, dest["p"], val[1])
    ke = np.bincount(dest["s"], minlength=ge0.shape[0]) + np.bincount(dest["o"], minlength=ge0.shape[0])
    kr = np.bincount(dest["p"], minlength=gr0.shape[0])
    if defect.get("overwrite"):  # the touched rows stored, not added to
        out = (np.where(ke[:, None] > 0, te, ge0), np.where(kr[:, None] > 0, tr, gr0))
    else:
        out = (ge0 + te, gr0 + tr)
    if not want_bound:
        return out, None
    ae, ar = np.abs(ge0), np.abs(gr0)
    _scatter(ae, S, comp[0])
    _scatter(ae, O, comp[2])
    _scatter(ar, P, comp[1])
    cs_, cp_, co_ = c_counts(name, lp, ent.shape[1])
    pre_e, pre_r = int(np.any(ge0 != 0)), int(np.any(gr0 != 0))
    be = np.where(ke[:, None] > 0, (ke[:, None] + pre_e + max(cs_, co_)) * U * ae, 0.0)
    br = np.where(kr[:, None] > 0, (kr[:, None] + pre_r + cp_) * U * ar, 0.0)
    return out, (be, br)


def expand(s, o, slot, neg):
    """the n K triples (S, O) of a negative-sampling call: `slot` (0 = s, 2 = o) of triple i replaced by neg[i, k]"""
    neg = np.asarray(neg).astype(np.int64)
    n, K = neg.shape
    rep = lambda x: np.repeat(np.asarray(x).astype(np.int64), K)
    return (neg.reshape(-1), rep(o)) if slot == 0 else (rep(s), neg.reshape(-1))


def spo_bwd(name, l_norm, ent, rel, s, p, o, gout, defect=None):
    defect = defect or {}
    Pg = np.roll(np.asarray(p), -1) if defect.get("rel_next") else p
    Sr, Rr, Or = _gather(name, ent, rel, s, Pg, o, defect)
    return _row_grads(name, float(l_norm), Sr, Rr, Or, np.asarray(gout, np.float64).reshape(-1),
                      float(defect.get("eps", EPS)), bool(defect.get("flip_cross")), False)[0]


def spo_bwd_bound(name, l_norm, ent, rel, s, p, o, gout):
    """one term per element: (1 + C) u A"""
    Sr, Rr, Or = _gather(name, ent, rel, s, p, o, {})
    comp = _row_grads(name, float(l_norm), Sr, Rr, Or, np.asarray(gout, np.float64).reshape(-1), EPS, False, True)[1]
    return tuple((1 + c) * U * a for c, a in zip(c_counts(name, l_norm, np.asarray(ent).shape[1]), comp))


def spo_bwd_accum(name, l_norm, ent, rel, s, p, o, gout, ge0, gr0, defect=None):
    return _accum(name, l_norm, ent, rel, s, p, o, gout, ge0, gr0, defect, False)[0]


def spo_bwd_accum_bound(name, l_norm, ent, rel, s, p, o, gout, ge0, gr0):
    return _accum(name, l_norm, ent, rel, s, p, o, gout, ge0, gr0, None, True)[1]


def neg_bwd_accum(name, l_norm, ent, rel, s, p, o, slot, neg, gout, ge0, gr0, defect=None):
    defect = dict(defect or {})
    if defect.pop("swap_slots", False):
        slot = 2 - slot
    S, O = expand(s, o, slot, neg)
    K = np.asarray(neg).shape[1]
    return _accum(name, l_norm, ent, rel, S, np.repeat(np.asarray(p).astype(np.int64), K), O, gout, ge0, gr0, defect,
                  False)[0]


def neg_bwd_accum_bound(name, l_norm, ent, rel, s, p, o, slot, neg, gout, ge0, gr0):
    S, O = expand(s, o, slot, neg)
    K = np.asarray(neg).shape[1]
    return _accum(name, l_norm, ent, rel, S, np.repeat(np.asarray(p).astype(np.int64), K), O, gout, ge0, gr0, None,
                  True)[1]


def reference(k):
    """(want, bound) of a made case in one evaluation: per-row triples for kind "spo", the two tables otherwise"""
    if k["kind"] == "spo":
        return spo_bwd(*ref_args(k)), spo_bwd_bound(*ref_args(k))
    S, P, O = triples_of(k)
    return _accum(k["name"], k["l_norm"], k["ent"], k["rel"], S, P, O, k["gout"], k["ge0"], k["gr0"], None, True)


def rotate_min_modulus(k):
    """min |q - o| over every scored triple and complex coordinate of a RotatE case"""
    acc = []
    S, P, O = triples_of(k)
    Sr, Rr, Or = _gather("rotate", k["ent"], k["rel"], S, P, O, {})
    _row_grads("rotate", 1.0, Sr, Rr, Or, np.ones(len(S)), EPS, False, False, acc)
    return min(acc)


def transe_ties(k):
    """number of (triple, coordinate) with s + r == o exactly"""
    S, P, O = triples_of(k)
    Sr, Rr, Or = _gather("transe", k["ent"], k["rel"], S, P, O, {})
    return int((Sr + Rr == Or).sum())


def triples_of(k):
    """the scored triples of a made case"""
    if k["kind"] == "neg":
        S, O = expand(k["s"], k["o"], k["slot"], k["neg"])
        return S, np.repeat(k["p"], k["K"]), O
    return k["s"], k["p"], k["o"]


# ---- the host launch rules of bwd.hip, restated ---------------------------------------------------------------------------
def neg_chunk(n, K):
    """negatives per wave of run_neg_bwd_accum / run_neg_bwd_accum_sorted (bwd_neg_accum_kernel, bwd_neg_fixed_kernel)"""
    return min(64, max(4, n * K // 8192))


def spo_chunk(n):
    """triples per wave of run_spo_bwd_accum (bwd_spo_accum_kernel)"""
    return min(32, max(1, n // 4096))


def sorted_nc(d):
    """coordinate pairs per lane of bwd_neg_sorted_kernel / bwd_neg_fixed_kernel; None: KGE_ERR_UNSUPPORTED"""
    hh = (d + 1) // 2
    return 4 if hh <= 256 else (8 if hh <= 512 else None)


SORT_CH = 32  # NGS_CH: occurrences per wave of bwd_neg_sorted_kernel


def _max_run(ids):
    ids = np.sort(np.asarray(ids).reshape(-1))
    if ids.size == 0:
        return 0
    edges = np.flatnonzero(np.diff(ids)) + 1
    return int(np.diff(np.concatenate([[0], edges, [ids.size]])).max())


def branches(k):
    """What a made case reaches, from the rules above"""
    n, d = k["n"], k["d"]
    if k["kind"] == "neg":
        K = k["K"]
        ch = neg_chunk(n, K)
        cpr = -(-K // ch)
        ids = np.sort(k["neg"].reshape(-1))
        # a run of the sorted order that begins and ends strictly inside 32-chunks and is longer than one
        edges = np.concatenate([[0], np.flatnonzero(np.diff(ids)) + 1, [ids.size]])
        inside = any(b - a > SORT_CH and a % SORT_CH and b % SORT_CH for a, b in zip(edges[:-1], edges[1:]))
        return dict(ch=ch, cpr=cpr, last=K - (cpr - 1) * ch, nc=sorted_nc(d), sorted_last=(n * K - 1) % SORT_CH + 1,
                    max_run=_max_run(ids), run_inside=bool(inside), odd=bool(d % 2))
    if k["kind"] == "acc":
        ch = spo_chunk(n)
        return dict(ch=ch, last=n - (-(-n // ch) - 1) * ch, nc=sorted_nc(d), run_s=_max_run_consecutive(k["s"]),
                    run_p=_max_run_consecutive(k["p"]), first_run_s=int(np.argmax(k["s"] != k["s"][0])) if n > 1 else 1)
    return dict(second_group=n > 4, strided=d > 128, odd=bool(d % 2))


def _max_run_consecutive(x):
    x = np.asarray(x)
    edges = np.concatenate([[0], np.flatnonzero(np.diff(x)) + 1, [x.size]])
    return int(np.diff(edges).max())


# ---- the fixed cases -------------------------------------------------------------------------------------------------------
def _neg(name, l_norm, n, K, d, E, **kw):
    return dict(kind="neg", name=name, l_norm=float(l_norm), n=n, K=K, d=d, E=E, **kw)


NEG_CASES = [
    _neg("distmult", 1, 1, 1, 1, 10), _neg("transe", 1, 1, 1, 1, 10),
    _neg("complex", 1, 1, 1, 2, 10), _neg("rotate", 1, 1, 1, 2, 10),
    _neg("distmult", 1, 19, 70, 33, 60), _neg("transe", 1, 19, 70, 33, 60),
    _neg("complex", 1, 19, 70, 40, 60), _neg("rotate", 1, 19, 70, 40, 60),
    _neg("complex", 1, 19, 70, 40, 60, pitched=True), _neg("transe", 2, 19, 70, 33, 60, pitched=True),
    _neg("complex", 1, 450, 130, 4, 100_000, hub=600), _neg("distmult", 1, 450, 130, 4, 100_000, hub=600),
    _neg("transe", 1, 450, 130, 4, 100_000, hub=600), _neg("rotate", 1, 450, 130, 4, 100_000, hub=600),
    _neg("distmult", 1, 4100, 130, 4, 300_000, hub=600), _neg("rotate", 1, 4100, 130, 4, 300_000, hub=600),
    _neg("complex", 1, 8200, 64, 2, 300_000, hub=600), _neg("transe", 1, 8200, 64, 2, 300_000, hub=600),
    _neg("complex", 1, 3, 40, 514, 40), _neg("rotate", 1, 3, 40, 514, 40),
    _neg("complex", 1, 3, 9, 1024, 20), _neg("rotate", 2, 3, 9, 1024, 20),
    _neg("distmult", 1, 3, 9, 1023, 20), _neg("transe", 1, 3, 9, 1023, 20),
    _neg("complex", 1, 37, 131, 64, 23, hub=60), _neg("rotate", 1, 37, 131, 64, 23, hub=60),
    _neg("transe", 1, 37, 131, 64, 23, hub=60),
    _neg("distmult", 1, 3, 11, 8, 30), _neg("rotate", 1, 3, 11, 8, 30),
    _neg("transe", 2, 5, 9, 2, 60, per=1), _neg("transe", 2, 5, 9, 130, 60),
    _neg("transe", 3, 5, 9, 2, 60, per=1), _neg("transe", 3, 5, 9, 33, 60), _neg("transe", 3, 5, 9, 130, 60),
    _neg("rotate", 2, 5, 9, 2, 60, per=1), _neg("rotate", 2, 5, 9, 66, 60), _neg("rotate", 2, 5, 9, 130, 60),
    _neg("rotate", 3, 5, 9, 2, 60, per=1), _neg("rotate", 3, 5, 9, 66, 60), _neg("rotate", 3, 5, 9, 130, 60),
]
NEG_UNSUPPORTED = _neg("complex", 1, 2, 5, 1026, 12)


def _spo(name, l_norm, n, d, **kw):
    return dict(kind="spo", name=name, l_norm=float(l_norm), n=n, d=d, E=14, **kw)


SPO_CASES = [
    _spo("distmult", 1, 1, 1), _spo("transe", 1, 1, 1), _spo("complex", 1, 4, 2), _spo("transe", 1, 4, 2),
    _spo("rotate", 2, 1, 2), _spo("transe", 1, 5, 33), _spo("distmult", 1, 4, 33), _spo("transe", 3, 4, 33),
    _spo("rotate", 1, 5, 66), _spo("transe", 3, 5, 66), _spo("rotate", 3, 1, 66), _spo("transe", 2, 4, 130),
    _spo("rotate", 3, 4, 130), _spo("rotate", 2, 5, 130), _spo("complex", 1, 5, 1024), _spo("rotate", 1, 1, 1024),
    _spo("transe", 2, 4, 1024),
]


def _acc(name, l_norm, n, d, E, **kw):
    return dict(kind="acc", name=name, l_norm=float(l_norm), n=n, d=d, E=E, **kw)


ACC_CASES = [
    _acc("complex", 1, 37, 40, 60, rs=2, rp=3), _acc("distmult", 1, 37, 40, 60, rs=2, rp=3),
    _acc("transe", 1, 37, 40, 60, rs=2, rp=3), _acc("rotate", 1, 37, 40, 60, rs=2, rp=3),
    _acc("transe", 2, 37, 40, 60, rs=2, rp=3, pitched=True), _acc("rotate", 3, 37, 40, 60, rs=2, rp=3),
    _acc("complex", 1, 37, 40, 60, rs=2, rp=3, pitched=True),
    _acc("complex", 1, 3 * 4096 + 5, 4, 50_000, rs=5, rp=7, hub=300),
    _acc("transe", 1, 3 * 4096 + 5, 4, 50_000, rs=5, rp=7, hub=300),
    _acc("distmult", 1, 32 * 4096 + 7, 2, 200_000, rs=45, rp=7, hub=300),
    _acc("rotate", 1, 32 * 4096 + 7, 2, 200_000, rs=45, rp=7, hub=300),
    _acc("complex", 1, 3, 1024, 12, rs=2, rp=2), _acc("transe", 1, 3, 1023, 12, rs=2, rp=2),
]
ACC_UNSUPPORTED = _acc("complex", 1, 3, 1026, 12, rs=2, rp=2)

ALL_CASES = NEG_CASES + SPO_CASES + ACC_CASES + [NEG_UNSUPPORTED, ACC_UNSUPPORTED]


def case_id(c):
    extra = "".join(f"-{k}{'' if v is True else v}" for k, v in c.items()
                    if k not in ("kind", "name", "l_norm", "n", "K", "E", "d"))
    norm = "" if c["name"] in ("complex", "distmult") else f"-L{c['l_norm']:g}"
    shape = f"n{c['n']}-K{c['K']}" if c["kind"] == "neg" else f"n{c['n']}"
    return f"{c['kind']}-{c['name']}{norm}-{shape}-d{c['d']}-E{c['E']}{extra}"


def _tables(rng, name, E, R, d, low_end):
    """The input families of _pairs_bwd_ref.make_case.  RotatE: rows 0..3 on four modulus levels 0.06 apart, rows
    4..low_end-1 moduli in [0.5, 0.72], rows from low_end on in [1, 1.5]: |q - o| >= 0.28 between a low and a high row,
    0.04 among rows 0..3, and phases 0.1 <= |r| <= pi keep a row 0.05 away from its own rotation."""
    dr = d // 2 if name == "rotate" else d
    if name in ("complex", "distmult"):
        return _mag(rng, (E, d)), _mag(rng, (R, dr))
    if name == "transe":  # the grid 2^-6 Z in [-2, 2]: s + r - o exact in float32 and float64
        return ((rng.integers(-128, 129, (E, d)) / 64.0).astype(np.float32),
                (rng.integers(-128, 129, (R, dr)) / 64.0).astype(np.float32))
    h = d // 2
    mod = rng.uniform(1.0, 1.5, (E, h))
    mod[:low_end] = rng.uniform(0.5, 0.72, (min(low_end, E), h))
    mod[:4] = 0.5 + 0.06 * np.arange(4)[:, None] + rng.uniform(0.0, 0.02, (4, h))
    ang = rng.uniform(-np.pi, np.pi, (E, h))
    ent = np.hstack([mod * np.cos(ang), mod * np.sin(ang)]).astype(np.float32)
    rel = (rng.uniform(0.1, 3.14, (R, dr)) * rng.choice([-1.0, 1.0], (R, dr))).astype(np.float32)
    return ent, rel


def make_case(c, slot=None, seed=None):
    """The inputs of one case (and slot, for a neg case): the case's fields plus ent [E, d], rel [R, d_r], s, p, o [n]
    (int64), gout, ge0 [E, d], gr0 [R, d_r] (the gradients' initial contents: zeros unless pre-loaded) and, for a neg
    case, neg [n, K] (int64), slot, tie_row."""
    name, n, d, E, kind = c["name"], c["n"], c["d"], c["E"], c["kind"]
    if seed is None:
        seed = 1000 * ALL_CASES.index(c) + (slot or 0)
    rng = np.random.default_rng(seed)
    out = dict(c)
    half = slice(0, (d + 1) // 2)
    if kind == "neg":
        K = c["K"]
        # at most 650 terms per fixed entity row and per relation row: `per` positives share one
        per = c.get("per") or max(1, 650 // K)
        groups = max(2, -(-n // per))
        R = groups if n > 1 else 1
        low_end = 4 + groups
        assert low_end + 3 <= E
        i = np.arange(n)
        s, o, p = 4 + i % groups, 4 + (i + 1) % groups, i % R
        s[0], o[0] = 0, 1  # the planted row: two of the levelled rows
        ent, rel = _tables(rng, name, E, R, d, low_end)
        tie_row = low_end
        neg = rng.integers(low_end + 1, E, (n, K))
        if c.get("hub"):  # one entity with a long run of the sorted order, one with a run of 40
            flat = neg.reshape(-1)
            pos = rng.choice(np.arange(K, n * K), c["hub"] + 40, replace=False)
            flat[pos[:c["hub"]]] = E - 1
            flat[pos[c["hub"]:]] = E - 2
        fixed, repl = (o[0], s[0]) if slot == 0 else (s[0], o[0])
        neg[0, 0] = tie_row
        if K >= 3:
            neg[0, 1], neg[0, 2] = fixed, repl  # the positive's own fixed entity, and the positive itself
        if name == "transe" and d == 1:
            # one coordinate, no tie: low rows 0.5, high rows 2 -- the varying (high) row decides the sign of s + r - o,
            # so that read as zero, or exchanged with the fixed row, it changes the weight
            ent[:low_end], ent[low_end:], rel[:] = 0.5, 2.0, (-0.5 if slot == 0 else 0.5)
        elif name == "transe":  # an exact tie in the first half of the coordinates of occurrence (0, 0)
            q = ent[o[0]] - rel[p[0]] if slot == 0 else ent[s[0]] + rel[p[0]]
            ent[tie_row, half] = q[half]
        gout = _mag(rng, (n, K))
        out.update(slot=slot, neg=neg.astype(np.int64), tie_row=tie_row)
    elif kind == "spo":
        R, low_end = 5, 6
        i = np.arange(n)
        s, o, p = i.copy(), low_end + 1 + i, i % R
        ent, rel = _tables(rng, name, E, R, d, low_end)
        if name == "transe" and d == 1:
            ent[:low_end], ent[low_end:], rel[:] = 0.5, 2.0, 0.5  # (as above)
        elif name == "transe":
            ent[o[0], half] = (ent[s[0]] + rel[p[0]])[half]
        gout = _mag(rng, (n,))
    else:
        rs, rp = c["rs"], c["rp"]
        i = np.arange(n)
        s, p = 4 + (i + rs - 1) // rs, (i + rp - 1) // rp  # runs of rs / rp triples, the first run one triple long
        R, low_end = int(p.max()) + 1, int(s.max()) + 1
        assert low_end + 3 <= E
        o = rng.integers(low_end, E, n)
        if c.get("hub"):
            o[rng.choice(np.arange(1, n), c["hub"], replace=False)] = E - 1
        ent, rel = _tables(rng, name, E, R, d, low_end)
        if name == "transe":
            ent[o[0], half] = (ent[s[0]] + rel[p[0]])[half]
        gout = _mag(rng, (n,))
    pre = bool(c.get("pitched"))
    dr = rel.shape[1]
    out.update(ent=ent, rel=rel, s=s.astype(np.int64), p=p.astype(np.int64), o=o.astype(np.int64), gout=gout, R=R,
               ge0=_mag(rng, (E, d)) if pre else np.zeros((E, d), np.float32),
               gr0=_mag(rng, (R, dr)) if pre else np.zeros((R, dr), np.float32), preloaded=pre)
    return out


def ref_args(k):
    a = (k["name"], k["l_norm"], k["ent"], k["rel"], k["s"], k["p"], k["o"])
    if k["kind"] == "neg":
        return a + (k["slot"], k["neg"], k["gout"], k["ge0"], k["gr0"])
    return a + ((k["gout"],) if k["kind"] == "spo" else (k["gout"], k["ge0"], k["gr0"]))
