"""The numpy restatement of the embedder-dropout mask (tests/_dropout_ref.py; include/kge_amd.h "Embedder dropout") and
of the dropout backward, without a GPU: keep rate and independence of the mask within 5-sigma binomial bounds on fixed
seeds, the threshold at its edges, and -- on the very inputs tests/test_gpu_dropout.py runs -- that a mask of the wrong
call, a missing mask factor on the gradient and a fixed row re-masked per negative each exceed the bound."""
import math

import numpy as np
import pytest

import _dropout_ref as dr

SEED = 0x0123_4567_89AB_CDEF


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    N, width = 1 << 20, 256
    f = dr.factor(N // width, width, 5, 3, dr.ROLE_S, SEED, p)
    kept = int((f != 0).sum())
    pf = float(np.float32(p))
    assert abs(kept / N - (1 - pf)) <= 5 * math.sqrt(pf * (1 - pf) / N), kept / N
    assert set(np.unique(f).tolist()) == {0.0, float(dr.scale(p))}


def _mask(p=0.5, occ0=0, call=1, role=0, seed=SEED):
    return dr.factor(256, 256, occ0, call, role, seed, p) == 0  # 2^16 elements


@pytest.mark.parametrize("other", [dict(role=2), dict(role=1), dict(occ0=256), dict(call=2), dict(seed=SEED + 1),
                                   dict(seed=SEED ^ (1 << 40))])
def test_masks_differ_and_are_uncorrelated(other):
    p, N = 0.5, 1 << 16
    a, b = _mask(), _mask(**other)
    assert (a != b).any()
    # both dropped: binomial(N, p^2)
    both = int((a & b).sum())
    assert abs(both / N - p * p) <= 5 * math.sqrt(p * p * (1 - p * p) / N), both / N
    # the sampler's streams of the same seed are other streams: the key differs
    assert dr.KEY_XOR == 0x44524F50


def test_occurrences_of_one_call_are_consecutive_rows():
    a = dr.factor(8, 40, 3, 9, 2, SEED, 0.3)
    b = dr.factor(4, 40, 5, 9, 2, SEED, 0.3)
    assert (a[2:6] == b).all()


def test_threshold_edges():
    assert dr.threshold(0.0) == 0 and dr.threshold(0.5) == 1 << 31 and dr.threshold(2.0 ** -32) == 1
    for k in (1, 2, 3, 1 << 8, (1 << 24) - 1):
        assert dr.threshold(k * 2.0 ** -32) == k  # exact in float32 up to 24 bits
    top = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert dr.threshold(top) == (1 << 32) - (1 << 8)
    # word < thr: word thr - 1 is dropped, word thr is kept -- and p == 0 keeps word 0
    w = dr.words(np.arange(64), 0, 1, 0, SEED)
    t = int(w[7])
    assert bool(w[7] < np.uint64(t + 1)) and not bool(w[7] < np.uint64(t))
    assert (dr.factor(3, 9, 0, 1, 0, SEED, 0.0) == 1).all()
    assert dr.scale(0.5) == np.float32(2.0) and dr.scale(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))


def test_embed_restatement_signs_and_bits():
    tab = np.array([[1.5, -2.0, 0.0, -0.0, 3.0, -4.0, 5.0, 6.0]], dtype=np.float32)
    out = dr.embed(tab, [0, 0, 0], 0, 1, 0, SEED, 0.5)
    f = dr.factor(3, 8, 0, 1, 0, SEED, 0.5)
    assert (out == tab * f).all() and (np.signbit(out) == np.signbit(np.broadcast_to(tab, out.shape))).all()
    assert (out[0] != out[1]).any()  # two occurrences of one row carry different masks
    assert dr.embed(tab, [0], 0, 1, 0, SEED, 0.0).tobytes() == tab.tobytes()


CASES = dr.bwd_cases()


@pytest.mark.parametrize("case", CASES, ids=dr.bwd_case_id)
def test_backward_reference_and_planted_defects(case):
    c, slot, p_ent, p_rel, seed, call = case
    k = dr.make_bwd_case(case)
    (ge, gr), (be, br), mod = dr.bwd_reference(k, p_ent, p_rel, seed, call)
    assert np.isfinite(ge).all() and np.isfinite(gr).all() and np.isfinite(be).all() and np.isfinite(br).all()
    if c["name"] == "rotate":
        assert mod >= 0.01, mod  # no complex coordinate of a masked triple collapses: the weights are conditioned
    trivial = k["n"] * k.get("K", 1) * c["d"] <= 4  # a handful of elements: a defect may leave every mask as it was
    for defect in dr.BWD_DEFECTS:
        if defect == "remask_fixed" and (k["kind"] != "neg" or k["K"] == 1):
            continue  # no fixed row
        (de, dr_), _, _ = dr.bwd_reference(k, p_ent, p_rel, seed, call, defect)
        worst = max(float(np.max(np.abs(de - ge) - be)), float(np.max(np.abs(dr_ - gr) - br)))
        if not trivial:
            assert worst > 0, (defect, worst)
