"""kge_score_neg_shared_bwd_accum (score_neg_shared.hip: sns_fold_base_kernel, sns_fold_repeat_kernel and both roles of
neg_shared_bwd_kernel) restated in numpy float64 for the tests (no torch, no GPU), with an elementwise rounding bound.

  samples(unique, drop, repeat, n) -> [n, K] ids: column c < Uc shows unique[c], or unique[Uc] (the spare) where
                                      drop[i] == c; column Uc + r shows column repeat[r] of the same row
  shared_bwd_accum(..., slot, unique, drop, repeat, gout, ge0, gr0)  IS _neg_bwd_ref.neg_bwd_accum on samples(...) and is
                                      computed so: row gradients, weights and C counts are that module's
  shared_bwd_accum_folded(...)        a second statement, the kernel's order: gout folded into one weight W[i, u] per
                                      (positive, physical row), then one term per pair.  It exists to show that the two
                                      agree and to carry the defects of the fold
  shared_bwd_accum_bound(...)         _neg_bwd_ref.neg_bwd_accum_bound on the materialised samples, unchanged

Bound, elementwise: |float32 result - reference| <= (K_e + C) u A_e with K_e, A_e and C of _neg_bwd_ref on the
materialised samples.  Why no new constant: the kernel sums Kp folded terms W[i, u] t(i, u) into a table element (register
partials over a tile, one atomic flush per (owner, tile): a float32 sum of Kp terms in some order, (Kp - 1) u), and the
largest fold behind one of them, W = a float32 sum of m values of gout in some order (the base store, then float atomics),
carries (m - 1) u sum |gout|; one term's own roundings are the C of spo_pair_grads, its weight and the stored distance
(the forward's scores, -scores[i, c] of the column that shows the pair: every column of a pair holds the same float32
score, the forward being a function of the two rows alone).  First order: (Kp - 1 + (m - 1) + C) u A.  The materialised
sum has K_e = sum of the m's over the element's pairs >= Kp + m_max - 1 terms, and |W| <= sum |gout| term by term, which
is how A_e counts them: (K_e + C) u A_e covers it.  A pair whose weights cancel (W == 0.f, skipped by the kernel) adds
exactly 0 on both sides.  An element no occurrence goes to has bound 0 and must equal its initial content as a NUMBER: the
kernel flushes a +0.f into the rows of owners whose pairs no column shows, which turns a -0.0 into +0.0 -- the pre-loaded
gradients here hold no -0.0.

shared_nc / role0_tile / role1_tile / OWNERS_PER_WG / OWNERS_PER_WAVE restate the host rules of
run_neg_shared_bwd_accum, `branches` evaluates them per case.  The fixed case list of tests/test_gpu_neg_shared_bwd.py is
built here (CASES, make_case, case_id) so that tests/test_neg_shared_bwd_ref_cpu.py checks the very inputs the GPU file
runs.  A made case carries kind = "neg", neg = samples(...) and K: _neg_bwd_ref.reference / triples_of / ref_args /
transe_ties / rotate_min_modulus take it as it is.
"""
import itertools

import numpy as np

import _neg_bwd_ref as NB
from _pairs_bwd_ref import _mag

OWNERS_PER_WAVE = 4                  # SNB_OPW
OWNERS_PER_WG = 4 * OWNERS_PER_WAVE  # SNB_OB
STAGE_FLOATS = 8192                  # SNB_SM


def shared_nc(d):
    """coordinate pairs per lane of neg_shared_bwd_kernel; None: KGE_ERR_UNSUPPORTED"""
    hh = (d + 1) // 2
    if hh > 64 * 8:
        return None
    nc = 1
    while 64 * nc < hh:
        nc <<= 1
    return nc


def role0_tile(nc):
    """physical rows staged per workgroup of ROLE 0 (owners: positives)"""
    return 64 // nc


def role1_tile(nc):
    """positives staged per workgroup of ROLE 1 (owners: physical rows)"""
    return 32 // nc


# ---- the definition ---------------------------------------------------------------------------------------------------------
def _ids(x):
    return np.zeros(0, np.int64) if x is None else np.asarray(x).astype(np.int64).reshape(-1)


def samples(unique, drop, repeat, n):
    unique, rep = _ids(unique), _ids(repeat)
    uc = unique.size - (0 if drop is None else 1)
    dr = None if drop is None else _ids(drop).tolist()
    base = np.empty((n, uc), np.int64)
    for i in range(n):
        for c in range(uc):
            base[i, c] = unique[uc] if dr is not None and dr[i] == c else unique[c]
    return np.hstack([base] + [base[:, [c]] for c in rep]) if rep.size else base


def physical(drop, repeat, n, uc):
    """[n, K]: the physical row (index into `unique`) each column of row i shows"""
    rep = _ids(repeat)
    ph = np.broadcast_to(np.arange(uc), (n, uc)).copy()
    if drop is not None:
        dr = _ids(drop)
        hit = np.flatnonzero(dr < uc)
        ph[hit, dr[hit]] = uc
    return np.hstack([ph, ph[:, rep]]) if rep.size else ph


def shared_bwd_accum(name, l_norm, ent, rel, s, p, o, slot, unique, drop, repeat, gout, ge0, gr0, defect=None):
    n = np.asarray(s).size
    return NB.neg_bwd_accum(name, l_norm, ent, rel, s, p, o, slot, samples(unique, drop, repeat, n), gout, ge0, gr0,
                            defect)


def shared_bwd_accum_bound(name, l_norm, ent, rel, s, p, o, slot, unique, drop, repeat, gout, ge0, gr0):
    n = np.asarray(s).size
    return NB.neg_bwd_accum_bound(name, l_norm, ent, rel, s, p, o, slot, samples(unique, drop, repeat, n), gout, ge0, gr0)


# ---- the kernel's order ------------------------------------------------------------------------------------------------------
def fold_weights(drop, repeat, gout, n, uc, defect=None):
    """W [n, P] of sns_fold_base_kernel + sns_fold_repeat_kernel.  Planted defects:
      base_ignores_drop    the dropped column's weight credited to the column's own row, not the spare
      repeat_ignores_drop  a repeat of a dropped column credited to the column's own row
      no_repeats           the repeat columns left out
      dup_once             a column named twice among the repeats counted once"""
    defect = defect or {}
    gout = np.asarray(gout, np.float64)
    rep = _ids(repeat)
    P = uc + (0 if drop is None else 1)
    dr = np.full(n, -1, np.int64) if drop is None else _ids(drop)
    rows = np.arange(n)
    W = np.zeros((n, P))
    for u in range(uc):
        own = np.ones(n, bool) if defect.get("base_ignores_drop") else dr != u
        W[own, u] = gout[own, u]
        if drop is not None and not defect.get("base_ignores_drop"):
            W[~own, uc] = gout[~own, u]
    if defect.get("no_repeats"):
        return W
    seen = set()
    for r, c in enumerate(rep):
        if defect.get("dup_once") and int(c) in seen:
            continue
        seen.add(int(c))
        to = np.full(n, c) if defect.get("repeat_ignores_drop") else np.where(dr == c, uc, c)
        np.add.at(W, (rows, to), gout[:, uc + r])
    return W


def _dist2(name, S, Rr, O):
    """the Euclidean distance of every row triple (l_norm 2), for the spare_dist_col0 defect only"""
    if name == "transe":
        return np.sqrt(((S + Rr - O + NB.EPS) ** 2).sum(1))
    h = S.shape[1] // 2
    q0 = S[:, :h] * np.cos(Rr) - S[:, h:] * np.sin(Rr)
    q1 = S[:, :h] * np.sin(Rr) + S[:, h:] * np.cos(Rr)
    return np.sqrt(((q0 - O[:, :h]) ** 2 + (q1 - O[:, h:]) ** 2).sum(1))


def shared_bwd_accum_folded(name, l_norm, ent, rel, s, p, o, slot, unique, drop, repeat, gout, ge0, gr0, defect=None):
    """W first, then one term per (positive, physical row): the n P pairs as triples weighted by W.  Further defect:
      spare_dist_col0      l_norm 2: the spare pair's distance read from column 0 instead of column drop[i] (the term is
                           proportional to 1 / dist)"""
    defect = defect or {}
    unique = _ids(unique)
    n = np.asarray(s).size
    uc = unique.size - (0 if drop is None else 1)
    P = unique.size
    W = fold_weights(drop, repeat, gout, n, uc, defect)
    S, O = NB.expand(s, o, slot, np.broadcast_to(unique, (n, P)))
    Pp = np.repeat(_ids(p), P)
    if defect.get("spare_dist_col0"):
        assert float(l_norm) == 2.0 and drop is not None
        e64, r64 = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
        dist = _dist2(name, e64[S], r64[Pp], e64[O]).reshape(n, P)
        col0 = np.where(_ids(drop) == 0, uc, 0)  # the row column 0 shows
        W = W.copy()
        W[:, uc] *= dist[:, uc] / dist[np.arange(n), col0]
    return NB._accum(name, l_norm, ent, rel, S, Pp, O, W.reshape(-1), ge0, gr0, None, False)[0]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
FOLDS = ("no_drop", "spare_never", "same_column", "mixed", "own_positive", "no_repeats", "dup_repeat",
         "repeat_of_dropped", "one_column", "cancel", "dup_unique", "own_entities")
NAMES = ("complex", "distmult", "transe", "rotate")


def _c(name, l_norm, n, uc, d, samp, **kw):
    return dict(name=name, l_norm=float(l_norm), n=n, Uc=uc, d=d, samp=samp, **kw)


def _both(name, l_norm, n, P, d, **kw):
    """naive and default sampling on the same number P of physical rows"""
    return [_c(name, l_norm, n, P, d, "naive", **kw), _c(name, l_norm, n, P - 1, d, "default", **kw)]


def _build_cases():
    out = []
    for name, d in (("distmult", 1), ("transe", 1), ("complex", 2), ("rotate", 2)):  # one element
        out += [_c(name, 1, 1, 1, d, "naive", nrep=0), _c(name, 1, 1, 1, d, "default", nrep=0)]
    for name in NAMES:  # nc = 1, the staging buffer full: tiles 64 + 1 rows, 32 + 1 positives
        out += _both(name, 1, 33, 65, 128)
    for j, (n, P) in enumerate(itertools.product((15, 16, 17), (63, 64, 65))):  # nc = 1: owner and tile edges
        out += _both(("complex", "rotate")[j % 2], 1, n, P, 40) + _both(("distmult", "transe")[j % 2], 1, n, P, 33)
    for name in NAMES:  # nc = 2, smallest: tiles 32 + 1 rows, 16 + 1 positives
        out += _both(name, 1, 17, 33, 130)
    for name in ("complex", "transe"):
        out += _both(name, 1, 17, 33, 256)
    for k, d in enumerate((258, 400, 512)):  # nc = 4: tiles of 16 rows and 8 positives
        for j, (n, P) in enumerate(itertools.product((7, 8, 9), (15, 16, 17))):
            out += _both(NAMES[(j + k) % 4], 1, n, P, d)
    for name in ("complex", "rotate"):  # nc = 8
        out += _both(name, 1, 5, 9, 514)
    for name in NAMES:
        out += _both(name, 1, 5, 9, 1024)  # full buffer: tiles 8 + 1 rows, 4 + 1 positives
    for name in ("distmult", "transe"):
        out += _both(name, 1, 5, 9, 1023)  # hh 512 / lim1 511
    for name in NAMES:  # long sums per physical row: 10 ROLE 1 tiles, one owner workgroup of 5 (+ 1)
        out += [_c(name, 1, 300, 5, 40, "naive", nrep=0), _c(name, 1, 300, 5, 40, "default", nrep=0)]
    for name in ("complex", "transe"):
        out += [_c(name, 1, 19, 70, 40, "naive" if f == "no_drop" else "default", fold=f) for f in FOLDS]
    for lp in (2, 3):
        out += [_c("transe", lp, 5, 7, d, "default", per=1, nrep=2) for d in (2, 33, 130)]
        out += [_c("rotate", lp, 5, 7, d, "default", per=1, nrep=2) for d in (2, 66, 130)]
    for samp in ("naive", "default"):
        out += [_c("complex", 1, 19, 70, 40, samp, pitched=True, nrep=9),
                _c("transe", 2, 19, 70, 33, samp, pitched=True, nrep=9)]
    return out


CASES = _build_cases()
UNSUPPORTED = [_c("complex", 1, 2, 5, 1026, "default", nrep=0), _c("distmult", 1, 2, 5, 1025, "naive", nrep=0)]


def case_id(c):
    extra = "".join(f"-{k}{'' if v is True else v}" for k, v in c.items()
                    if k not in ("name", "l_norm", "n", "Uc", "d", "samp"))
    norm = "" if c["name"] in ("complex", "distmult") else f"-L{c['l_norm']:g}"
    return f"{c['name']}{norm}-n{c['n']}-Uc{c['Uc']}-d{c['d']}-{c['samp']}{extra}"


def _repeats(c, rng, uc, default):
    fold = c.get("fold")
    if fold == "no_repeats" or uc == 0:
        return np.zeros(0, np.int64)
    if fold == "one_column":
        return np.full(40, 7, np.int64)
    if fold == "repeat_of_dropped":
        return np.array([5, 11, 23], np.int64)
    if fold == "cancel":
        return np.array([9, 30], np.int64)
    nrep = c.get("nrep", 9 if fold else (3 if default else 0))
    rep = rng.integers(0, uc, nrep).astype(np.int64)
    if nrep >= 2:
        rep[1] = rep[0]  # a duplicate among the repeats
    return rep


def make_case(c, slot, seed=None):
    """The inputs of one case and slot: the case's fields plus ent [E, d], rel [R, d_r], s, p, o [n], unique [P], drop [n]
    or None, repeat [nrep] (all int64), gout [n, K], ge0, gr0 (the gradients' initial contents: zeros unless pre-loaded),
    neg = samples(unique, drop, repeat, n), K, P, E, R, tie_row, kind = "neg" (see the module docstring)."""
    name, n, d, uc = c["name"], c["n"], c["d"], c["Uc"]
    default, fold = c["samp"] == "default", c.get("fold")
    if seed is None:
        seed = 1000 * (CASES + UNSUPPORTED).index(c) + slot
    rng = np.random.default_rng(seed)
    P = uc + (1 if default else 0)
    rep = _repeats(c, rng, uc, default)
    K = uc + rep.size
    # at most 650 terms per fixed entity row and per relation row: `per` positives share one
    per = c.get("per") or max(1, 650 // K)
    groups = max(2, -(-n // per))
    R = groups if n > 1 else 1
    low_end = 4 + groups
    tie_row = low_end
    E = low_end + 1 + P + 6
    i = np.arange(n)
    s, o, p = 4 + i % groups, 4 + (i + 1) % groups, i % R
    s[0], o[0] = 0, 1  # the planted row: two of the levelled rows
    fixed, repl = (o, s) if slot == 0 else (s, o)
    ent, rel = NB._tables(rng, name, E, R, d, low_end)
    # physical rows: the tie row first, then distinct high rows
    unique = np.concatenate([[tie_row], low_end + 1 + rng.permutation(E - low_end - 1)[:P - 1]]).astype(np.int64)
    drop = None
    if default:
        drop = rng.integers(0, uc + 1, n).astype(np.int64)  # mixed, the "no spare" value included
        if fold == "spare_never":
            drop[:] = uc
        elif fold == "same_column":
            drop[:] = uc - 1
        elif fold == "repeat_of_dropped":
            drop[1], drop[n - 1] = 5, 5
        elif fold == "one_column":
            drop[2] = 7
        elif fold == "cancel":
            drop[3] = 9  # the cancelling pair is the spare's there
        if fold not in ("spare_never", "same_column"):
            if n >= 4:
                drop[n - 2] = uc  # the "no spare" value is among them
            if n > 1 and drop[0] == 0:
                drop[0] = uc  # positive 0 keeps column 0: the planted tie
    assert fold not in ("own_positive", "own_entities") or name != "rotate"  # (two low rows: no modulus floor)
    if fold == "own_positive":  # the first replaced entities in the list, dropped by the rows they belong to
        mine = np.unique(repl)[:6]
        unique[2:2 + mine.size] = mine
        where = {int(e): 2 + j for j, e in enumerate(mine)}
        for r in range(n):
            if int(repl[r]) in where:
                drop[r] = where[int(repl[r])]
    if fold == "own_entities":  # positive 0's own fixed entity and its own replaced entity
        unique[1], unique[2] = fixed[0], repl[0]
    if fold == "dup_unique":  # two physical rows, one table row
        unique[5] = unique[4]
    if name == "transe" and d == 1:
        # one coordinate, no tie: low rows 0.5, high rows 2 -- the varying (high) row decides the sign of s + r - o
        ent[:low_end], ent[low_end:], rel[:] = 0.5, 2.0, (-0.5 if slot == 0 else 0.5)
    elif name == "transe":  # an exact tie in the first half of the coordinates of pair (0, column 0)
        half = slice(0, (d + 1) // 2)
        q = ent[o[0]] - rel[p[0]] if slot == 0 else ent[s[0]] + rel[p[0]]
        ent[tie_row, half] = q[half]
        # ... and its last coordinate one grid step past q: the sign of s + r - o there turns over if the physical row's
        # last coordinate is read as zero (15 rows against 3 queries may hold no such coordinate by chance)
        ql = float(q[d - 1])
        ent[tie_row, d - 1] = ql + (1.0 if ql > 0 or (ql == 0 and slot == 2) else -1.0) / 64.0
    gout = _mag(rng, (n, K))
    if fold == "cancel":  # column 9 weighs +g, its repeat -g: W == 0 exactly on a pair that columns do show
        gout[:, uc] = -gout[:, 9]
    pre = bool(c.get("pitched"))
    dr = rel.shape[1]
    out = dict(c)
    out.update(kind="neg", slot=slot, K=K, P=P, E=E, R=R, tie_row=tie_row, ent=ent, rel=rel, s=s.astype(np.int64),
               p=p.astype(np.int64), o=o.astype(np.int64), unique=unique, drop=drop, repeat=rep, gout=gout,
               ge0=_mag(rng, (E, d)) if pre else np.zeros((E, d), np.float32),
               gr0=_mag(rng, (R, dr)) if pre else np.zeros((R, dr), np.float32), preloaded=pre)
    out["neg"] = samples(unique, drop, rep, n)
    return out


def shared_args(k):
    return (k["name"], k["l_norm"], k["ent"], k["rel"], k["s"], k["p"], k["o"], k["slot"], k["unique"], k["drop"],
            k["repeat"], k["gout"], k["ge0"], k["gr0"])


def fold_features(k):
    """the features of the fold a made case carries, from its data"""
    n, uc, P = k["n"], k["Uc"], k["P"]
    drop, rep, unique = k["drop"], k["repeat"], k["unique"]
    repl = k["s"] if k["slot"] == 0 else k["o"]
    fixed = k["o"] if k["slot"] == 0 else k["s"]
    f = set()
    if drop is None:
        f.add("no_drop")
    else:
        if (drop == uc).all():
            f.add("spare_never")
        elif (drop == drop[0]).all():
            f.add("same_column")
        elif np.unique(drop).size > 1 and (drop == uc).any():
            f.add("mixed")
        if any(drop[i] < uc and unique[drop[i]] == repl[i] for i in range(n)):
            f.add("own_positive")
        if any(int(c) in set(drop.tolist()) for c in rep):
            f.add("repeat_of_dropped")
    if rep.size == 0:
        f.add("no_repeats")
    else:
        if np.unique(rep).size < rep.size:
            f.add("dup_repeat")
        if rep.size >= 40 and np.unique(rep).size == 1:
            f.add("one_column")
    if np.unique(unique).size < unique.size:
        f.add("dup_unique")
    if fixed[0] in unique and repl[0] in unique:
        f.add("own_entities")
    W = fold_weights(drop, rep, k["gout"], n, uc)
    ph = physical(drop, rep, n, uc)
    shown = np.zeros((n, P), bool)
    shown[np.repeat(np.arange(n), ph.shape[1]), ph.reshape(-1)] = True
    if (shown & (W == 0.0)).any():
        f.add("cancel")
    return frozenset(f)


def branches(k):
    """What a made case reaches, from the host rules above"""
    n, P, d, dr = k["n"], k["P"], k["d"], k["rel"].shape[1]
    nc = shared_nc(d)
    t0, t1 = role0_tile(nc), role1_tile(nc)
    r0_tiles, r1_tiles = -(-P // t0), -(-n // t1)
    r0_wgs, r1_wgs = -(-n // OWNERS_PER_WG), -(-P // OWNERS_PER_WG)
    return dict(nc=nc, r0_tiles=r0_tiles, r0_last=P - (r0_tiles - 1) * t0, r1_tiles=r1_tiles,
                r1_last=n - (r1_tiles - 1) * t1, r0_wgs=r0_wgs, r0_owners_last=n - (r0_wgs - 1) * OWNERS_PER_WG,
                r1_wgs=r1_wgs, r1_owners_last=P - (r1_wgs - 1) * OWNERS_PER_WG,
                full0=min(P, t0) * d == STAGE_FLOATS, full1=min(n, t1) * (d + dr) == STAGE_FLOATS, odd=bool(d % 2),
                fold=fold_features(k))
