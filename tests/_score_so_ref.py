"""kge_score_so / kge_score_so_bwd_accum (score_so.hip) restated in numpy float64 for the tests (no torch, no GPU), with
an elementwise rounding bound.

  triples(s, o, rels, R)            the n m triples (S, P, O) the [n, m] block stands for, row-major: (s[i], rels[j], o[i])
  scores(name, l_norm, ent, rel, s, o, rels=None) -> [n, m] float64, the scorer definitions of oracle/torch_port.py
                                    (score_emb, combine "spo") on those triples
  scores_bound(...)                 -> [n, m]: |float32 score - scores| <= bound
  bwd_accum(..., gout, ge0, gr0)    IS _neg_bwd_ref.spo_bwd_accum on triples(...) weighted by gout.reshape(-1), and is
                                    computed so
  bwd_accum_bound(...)              _neg_bwd_ref.spo_bwd_accum_bound on the same triples, unchanged

Gradient bound, elementwise: |float32 result - reference| <= (K_e + C) u A_e with K_e, A_e and C of _neg_bwd_ref.  Why no
new constant: the kernel adds K_e terms g t(i, j) into a table element -- register partials over a tile of relation
rows (ROLE 0) or of pairs (ROLE 1), then one float atomic per (owner, tile): a float32 sum of K_e terms in SOME order,
(K_e - 1) u, + 1 where the buffer was pre-loaded.  One term's own roundings are the C of spo_pair_grads with ROTPRE (the
same sincos_canon values, read from the LDS tile or the owner's registers), its weight and -- for l_norm != 1 -- the
stored distance, which is the forward score of kge_score_so = the bits of kge_score_spo (spo_device.hpp).  s[i] == o[i]
puts two terms of one pair into one element, a repeated pair or a repeated rels entry repeats terms: K_e counts every
one.  An element no index names has bound 0 and must keep its pre-loaded bits.

Score bound: a float32 score is a sum of Dn non-negative-magnitude terms in some order, each with c roundings of its
own: (Dn - 1 + c) u A, A the same sum on magnitudes; the p-th root of the distance scorers adds its own roundings
relative to the result (2 for sqrt or powf with its rounded exponent, covered by + 4).  It is used against the float32
torch port at the tolerance of tests/test_oracle_vs_reference.py; the GPU forward is compared with kge_score_spo bit
for bit and needs no bound.

The fixed case list of tests/test_gpu_score_so.py is built here (BWD_CASES, make_case, case_id) so that
tests/test_score_so_ref_cpu.py checks the very inputs the GPU file runs.
"""
import itertools

import numpy as np

import _neg_bwd_ref as NB
from _pairs_bwd_ref import U, _mag

NAMES = ("complex", "distmult", "transe", "rotate")
EPS = NB.EPS


def _ids(x):
    return np.asarray(x).astype(np.int64).reshape(-1)


def triples(s, o, rels, R):
    s, o = _ids(s), _ids(o)
    rels = np.arange(R, dtype=np.int64) if rels is None else _ids(rels)
    n, m = s.size, rels.size
    return np.repeat(s, m), np.tile(rels, n), np.repeat(o, m)


def _terms(name, l_norm, ent, rel, S, P, O):
    """per triple and reduction coordinate: (the term summed before the root, its magnitude companion, roundings)"""
    e, r = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    Sr, Rr, Or = e[S], r[P], e[O]
    lp = float(l_norm)
    if name == "distmult":
        return Sr * Rr * Or, np.abs(Sr * Rr * Or), 2
    h = Sr.shape[1] // 2
    if name == "complex":
        s0, s1, r0, r1, o0, o1 = Sr[:, :h], Sr[:, h:], Rr[:, :h], Rr[:, h:], Or[:, :h], Or[:, h:]
        t = (s0 * r0 - s1 * r1) * o0 + (s1 * r0 + s0 * r1) * o1
        a = (np.abs(s0 * r0) + np.abs(s1 * r1)) * np.abs(o0) + (np.abs(s1 * r0) + np.abs(s0 * r1)) * np.abs(o1)
        return t, a, 4
    if name == "transe":
        df = np.abs(Sr + Rr - Or + EPS)
        a = np.abs(Sr) + np.abs(Rr) + np.abs(Or) + EPS
        return df ** lp, np.maximum(df, a * 4 * U) ** (lp - 1) * a * max(lp, 1.0), 3 + 2
    s0, s1, o0, o1 = Sr[:, :h], Sr[:, h:], Or[:, :h], Or[:, h:]
    cs, sn = np.cos(Rr), np.sin(Rr)
    q0, q1 = s0 * cs - s1 * sn, s0 * sn + s1 * cs
    ab = np.sqrt((q0 - o0) ** 2 + (q1 - o1) ** 2)
    a = np.abs(s0) + np.abs(s1) + np.maximum(np.abs(o0), np.abs(o1))
    return ab ** lp, np.maximum(ab, a * 8 * U) ** (lp - 1) * 2 * a * max(lp, 1.0), 8 + 2


def scores(name, l_norm, ent, rel, s, o, rels=None):
    S, P, O = triples(s, o, rels, np.asarray(rel).shape[0])
    t, _, _ = _terms(name, l_norm, ent, rel, S, P, O)
    acc = t.sum(1)
    if name in ("transe", "rotate"):
        acc = -(acc ** (1.0 / float(l_norm)))
    return acc.reshape(_ids(s).size, -1)


def scores_bound(name, l_norm, ent, rel, s, o, rels=None):
    S, P, O = triples(s, o, rels, np.asarray(rel).shape[0])
    t, a, c = _terms(name, l_norm, ent, rel, S, P, O)
    dn = t.shape[1]
    b = (dn - 1 + c) * U * a.sum(1)
    if name in ("transe", "rotate"):
        lp = float(l_norm)
        acc = np.maximum(t.sum(1), 1e-300)
        # d (acc^(1/p)) = acc^(1/p - 1) / p d acc, + the root's own roundings relative to the result
        b = acc ** (1.0 / lp - 1.0) / lp * b + 4 * U * acc ** (1.0 / lp)
    return b.reshape(_ids(s).size, -1)


def bwd_accum(name, l_norm, ent, rel, s, o, rels, gout, ge0, gr0):
    S, P, O = triples(s, o, rels, np.asarray(rel).shape[0])
    return NB.spo_bwd_accum(name, l_norm, ent, rel, S, P, O, np.asarray(gout).reshape(-1), ge0, gr0)


def bwd_accum_bound(name, l_norm, ent, rel, s, o, rels, gout, ge0, gr0):
    S, P, O = triples(s, o, rels, np.asarray(rel).shape[0])
    return NB.spo_bwd_accum_bound(name, l_norm, ent, rel, S, P, O, np.asarray(gout).reshape(-1), ge0, gr0)


def owned_rows(s, o, rels, E, R):
    """(entity rows, relation rows) some index names, as boolean masks"""
    S, P, O = triples(s, o, rels, R)
    me, mr = np.zeros(E, bool), np.zeros(R, bool)
    me[S], me[O], mr[P] = True, True, True
    return me, mr


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def scalar_dim(name):
    """a dim the vector path does not take: 15 coordinates, or 2 x 7 for the complex scorers"""
    return 14 if name in ("complex", "rotate") else 15


def _c(name, l_norm, n, m, d, listed):
    return dict(name=name, l_norm=float(l_norm), n=n, m=m, d=d, listed=listed)


def _build_cases():
    out = []
    for name in NAMES:
        for d in (16, scalar_dim(name), 72):
            for (n, m), listed in itertools.product(((1, 5), (33, 5), (1, 33), (33, 33)), (False, True)):
                out.append(_c(name, 1, n, m, d, listed))
    for name, lp in itertools.product(("transe", "rotate"), (2, 3)):
        out += [_c(name, lp, 33, 33, 16, True), _c(name, lp, 33, 5, scalar_dim(name), False)]
    return out


BWD_CASES = _build_cases()


def case_id(c):
    norm = "" if c["name"] in ("complex", "distmult") else f"-L{c['l_norm']:g}"
    return f"{c['name']}{norm}-n{c['n']}-m{c['m']}-d{c['d']}-{'listed' if c['listed'] else 'all'}"


def make_case(c, seed=None):
    """The inputs of one case: the case's fields plus ent [E, d], rel [R, d_r] (the input families of
    _neg_bwd_ref._tables: TransE on a grid, RotatE subjects on low and objects on high moduli), s, o [n], rels ([m] or
    None), gout [n, m], ge0, gr0 (pre-loaded, no zeros).  With n >= 2: pair 0 has s == o, pair n - 1 repeats pair 1.  A
    listed `rels` is unsorted, repeats an id (m >= 2) and leaves 3 relation rows unnamed; 3 low and 3 high entity rows
    are never named."""
    name, n, m, d = c["name"], c["n"], c["m"], c["d"]
    if seed is None:
        seed = 7000 + BWD_CASES.index(c) if c in BWD_CASES else 1
    rng = np.random.default_rng(seed)
    nlow, nhigh = 6, 7
    low_end = 4 + nlow + 3          # rows 4 .. 4 + nlow - 1 are subjects, the next 3 low rows are never named
    E = low_end + nhigh + 3         # rows low_end .. low_end + nhigh - 1 are objects, the last 3 never named
    R = m + 3 if c["listed"] else m
    ent, rel = NB._tables(rng, name, E, R, d, low_end)
    i = np.arange(n)
    s = (4 + i % nlow).astype(np.int64)
    o = (low_end + (3 * i + 1) % nhigh).astype(np.int64)
    if n >= 2:
        o[0] = s[0]
        s[n - 1], o[n - 1] = s[1], o[1]
    rels = None
    if c["listed"]:
        rels = rng.permutation(R)[:m].astype(np.int64)
        if m >= 2:
            rels[m - 1] = rels[0]
    out = dict(c)
    out.update(E=E, R=R, ent=ent, rel=rel, s=s, o=o, rels=rels, gout=_mag(rng, (n, m)), ge0=_mag(rng, (E, d)),
               gr0=_mag(rng, (R, rel.shape[1])))
    return out


def ref_args(k):
    return (k["name"], k["l_norm"], k["ent"], k["rel"], k["s"], k["o"], k["rels"], k["gout"], k["ge0"], k["gr0"])
