"""numpy restatement of the embedder-dropout mask of include/kge_amd.h ("Embedder dropout"; kge_amd/csrc/philox.hpp is
the device form), and the float64 reference of the dropout backward entries built on tests/_neg_bwd_ref.py.

Element c of a gathered row occurrence is DROPPED iff word (c % 4) of Philox4x32-10(counter, key) < thr with
  counter = (c / 4, occ, (uint32)call, role)        role 0 = s row, 1 = p row, 2 = o row
  key     = (seed low 32, (seed high 32) ^ 0x44524F50)
  thr     = (uint32)floor(p * 2^32)                 (p: the float32 probability, widened to double)
kept -> x * scale, scale = float32(1) / (float32(1) - p); dropped -> x * 0.0f."""
import math

import numpy as np

from _neg_sample_ref import philox4x32_10

KEY_XOR = 0x44524F50
ROLE_S, ROLE_P, ROLE_O = 0, 1, 2


def threshold(p) -> int:
    """(uint32)floor(p * 2^32) in double, of the float32 value of p"""
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def scale(p) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(cols, occ, call, role, seed):
    """the 32-bit word that decides column `cols` of occurrence `occ` (arrays broadcast together) -> uint64 array"""
    seed = int(seed) & (2 ** 64 - 1)
    cols = np.asarray(cols, dtype=np.int64)
    occ = np.asarray(occ, dtype=np.int64)
    cols, occ = np.broadcast_arrays(cols, occ)
    r = philox4x32_10(cols >> 2, occ, int(call) & 0xFFFFFFFF, int(role), seed & 0xFFFFFFFF, (seed >> 32) ^ KEY_XOR)
    w = cols & 3
    return np.where(w == 0, r[0], np.where(w == 1, r[1], np.where(w == 2, r[2], r[3])))


def dropped(cols, occ, call, role, seed, p):
    """bool array: True where the element is dropped"""
    return words(cols, occ, call, role, seed) < np.uint64(threshold(p))


def factor(n, width, occ0, call, role, seed, p) -> np.ndarray:
    """float32 [n, width]: the mask factor (0 or scale) of the occurrences occ0 .. occ0 + n; p == 0: all ones"""
    if float(p) == 0.0:
        return np.ones((n, width), dtype=np.float32)
    occ = (np.arange(n, dtype=np.int64) + int(occ0))[:, None]
    drop = dropped(np.arange(width, dtype=np.int64)[None, :], occ, call, role, seed, p)
    return np.where(drop, np.float32(0.0), scale(p)).astype(np.float32)


def embed(table: np.ndarray, idx, occ0, call, role, seed, p) -> np.ndarray:
    """kge_embed_dropout: float32 [n, width], bit for bit (one float32 multiply per element; p == 0: a plain gather)"""
    rows = np.asarray(table, dtype=np.float32)[np.asarray(idx, dtype=np.int64)]
    if float(p) == 0.0:
        return rows.copy()
    return (rows * factor(len(rows), rows.shape[1], occ0, call, role, seed, p)).astype(np.float32)


def factor_at(occ, width, call, role, seed, p) -> np.ndarray:
    """float32 [len(occ), width]: the mask factors of the listed occurrences"""
    occ = np.asarray(occ, dtype=np.int64)
    if float(p) == 0.0:
        return np.ones((len(occ), width), dtype=np.float32)
    drop = dropped(np.arange(width, dtype=np.int64)[None, :], occ[:, None], call, role, seed, p)
    return np.where(drop, np.float32(0.0), scale(p)).astype(np.float32)


# ---- the dropout backward entries in float64 (kge_score_spo_dropout_bwd_accum, kge_score_neg_dropout_bwd_accum) --------
# The closed forms and companions of tests/_neg_bwd_ref.py (_row_grads) evaluated on the MASKED rows (the float32 products
# x * factor the kernels form, taken as exact inputs), each row gradient multiplied by its mask factor, scatter-added in
# float64.  Bound, elementwise, as _neg_bwd_ref._accum counts it: (K_e + pre + C + 1) u A_e -- C the roundings of one
# term of the undropped row gradient, + 1 for the extra float32 multiply by the factor (u |term|: the companion times the
# factor bounds |term|), K_e the number of terms added into the element (any summation order: the fixed rows' register
# sums multiplied once at the flush are (sum) * f, one more rounding of a magnitude below the sum of the terms'), A_e the
# companions times the factor summed, plus |initial content|.
BWD_DEFECTS = ("wrong_call", "no_factor", "remask_fixed")


def occurrences(k):
    """per scored triple the occurrence numbers of its (s, p, o) rows: the semantics of include/kge_amd.h"""
    n = k["n"]
    if k["kind"] != "neg":
        i = np.arange(n, dtype=np.int64)
        return i, i, i
    K = k["K"]
    fixed, var = np.repeat(np.arange(n, dtype=np.int64), K), np.arange(n * K, dtype=np.int64)
    return (var, fixed, fixed) if k["slot"] == 0 else (fixed, fixed, var)


def bwd_reference(k, p_ent, p_rel, seed, call, defect=None):
    """(grad_ent, grad_rel), (bound_ent, bound_rel), min RotatE modulus (or None) of a made case of _neg_bwd_ref under
    dropout.  defect: one of BWD_DEFECTS (then the bounds are None)."""
    import _neg_bwd_ref as nb
    name, lp = k["name"], float(k["l_norm"])
    S, P, O = (np.asarray(x).astype(np.int64) for x in nb.triples_of(k))
    occ_s, occ_p, occ_o = occurrences(k)
    if defect == "remask_fixed":  # a fixed row masked anew per negative
        occ_s = occ_p = occ_o = np.arange(len(S), dtype=np.int64)
    mcall = call + 1 if defect == "wrong_call" else call
    ent, rel = np.asarray(k["ent"], np.float32), np.asarray(k["rel"], np.float32)
    Fs = factor_at(occ_s, ent.shape[1], mcall, ROLE_S, seed, p_ent)
    Fp = factor_at(occ_p, rel.shape[1], mcall, ROLE_P, seed, p_rel)
    Fo = factor_at(occ_o, ent.shape[1], mcall, ROLE_O, seed, p_ent)
    Sr, Rr, Or = ((ent[S] * Fs).astype(np.float64), (rel[P] * Fp).astype(np.float64), (ent[O] * Fo).astype(np.float64))
    g = np.asarray(k["gout"], np.float64).reshape(-1)
    min_ab = []
    val, comp = nb._row_grads(name, lp, Sr, Rr, Or, g, nb.EPS, False, defect is None, min_ab)
    F = (Fs.astype(np.float64), Fp.astype(np.float64), Fo.astype(np.float64))
    if defect != "no_factor":
        val = tuple(v * f for v, f in zip(val, F))
    ge0, gr0 = np.asarray(k["ge0"], np.float64), np.asarray(k["gr0"], np.float64)
    te, tr = np.zeros_like(ge0), np.zeros_like(gr0)
    nb._scatter(te, S, val[0])
    nb._scatter(te, O, val[2])
    nb._scatter(tr, P, val[1])
    out = (ge0 + te, gr0 + tr)
    mod = min(min_ab) if min_ab else None
    if defect is not None:
        return out, None, mod
    comp = tuple(c * f for c, f in zip(comp, F))
    ae, ar = np.abs(ge0), np.abs(gr0)
    nb._scatter(ae, S, comp[0])
    nb._scatter(ae, O, comp[2])
    nb._scatter(ar, P, comp[1])
    ke = np.bincount(S, minlength=ge0.shape[0]) + np.bincount(O, minlength=ge0.shape[0])
    kr = np.bincount(P, minlength=gr0.shape[0])
    cs_, cp_, co_ = nb.c_counts(name, lp, ent.shape[1])
    pre_e, pre_r = int(np.any(ge0 != 0)), int(np.any(gr0 != 0))
    be = np.where(ke[:, None] > 0, (ke[:, None] + pre_e + max(cs_, co_) + 1) * nb.U * ae, 0.0)
    br = np.where(kr[:, None] > 0, (kr[:, None] + pre_r + cp_ + 1) * nb.U * ar, 0.0)
    return out, (be, br), mod


def bwd_cases():
    """The fixed cases of tests/test_gpu_dropout.py's backward tests: (case of _neg_bwd_ref, slot or None, p_ent, p_rel,
    seed, call).  TransE keeps its tables on the grid 2^-6 Z under scales that are powers of two (p = 0.5 / 0.75), so that
    the sign of s + r - o stays exact; RotatE drops few entity elements (p_ent = 2^-4) on seeds for which no complex
    coordinate has |q - o| below 0.01 (tests/test_dropout_ref_cpu.py asserts it)."""
    import _neg_bwd_ref as nb
    neg, acc = nb._neg, nb._acc
    out = []
    for c in (neg("distmult", 1, 19, 70, 33, 60), neg("complex", 1, 19, 70, 40, 60, pitched=True),
              neg("transe", 1, 19, 70, 33, 60), neg("transe", 2, 19, 70, 33, 60, pitched=True),
              neg("transe", 3, 5, 9, 130, 60), neg("rotate", 1, 19, 70, 40, 60), neg("rotate", 2, 5, 9, 66, 60),
              neg("rotate", 3, 5, 9, 130, 60), neg("complex", 1, 3, 9, 1024, 20), neg("distmult", 1, 3, 9, 1023, 20),
              neg("complex", 1, 1, 1, 2, 10), neg("distmult", 1, 37, 131, 6, 60)):
        for slot in (0, 2):
            out.append((c, slot))
    for c in (acc("complex", 1, 37, 40, 60, rs=2, rp=3), acc("distmult", 1, 37, 40, 60, rs=2, rp=3, pitched=True),
              acc("transe", 1, 37, 40, 60, rs=2, rp=3), acc("transe", 2, 37, 40, 60, rs=2, rp=3, pitched=True),
              acc("rotate", 1, 37, 40, 60, rs=2, rp=3), acc("rotate", 3, 37, 40, 60, rs=2, rp=3),
              acc("complex", 1, 3, 1024, 12, rs=2, rp=2), acc("transe", 1, 3, 1023, 12, rs=2, rp=2)):
        out.append((c, None))
    cases = []
    for j, (c, slot) in enumerate(out):
        if c["name"] == "transe":
            p_ent, p_rel = 0.5, 0.75
        elif c["name"] == "rotate":
            p_ent, p_rel = 0.0625, 0.3
        else:
            p_ent, p_rel = (0.3, 0.1) if j % 2 == 0 else (0.0, 0.2)
        cases.append((c, slot, p_ent, p_rel, 0x1234_5678_9ABC_DEF0 + j + 1000 * ROTATE_SEED_STEPS.get(j, 0), 7 + j))
    return cases


ROTATE_SEED_STEPS = {10: 17, 14: 1}  # (the RotatE cases whose first seed leaves a modulus below 0.02)


def make_bwd_case(case):
    import _neg_bwd_ref as nb
    c, slot = case[0], case[1]
    k = nb.make_case(c, slot=slot, seed=4242 + 17 * (slot or 0) + c["d"] + c["n"])
    if c["name"] == "rotate" and c["kind"] == "neg" and c["K"] >= 3:
        # make_case plants the positive's own entities as negatives: with a dropped phase (r = 0: q = s) and both
        # elements kept, q - o would vanish exactly there and the weight (q - o) / |q - o| has no reference value
        k["neg"][0, 1] = k["neg"][0, 2] = k["tie_row"]
    return k


def bwd_case_id(case):
    import _neg_bwd_ref as nb
    c, slot = case[0], case[1]
    return nb.case_id(c) + ("" if slot is None else f"-slot{slot}") + f"-p{case[2]:g}_{case[3]:g}"
