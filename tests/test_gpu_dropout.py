"""Embedder dropout inside the triple-wise kernels (include/kge_amd.h "Embedder dropout") on the GPU.

  mask      kge_embed_dropout is bit-equal to the numpy restatement tests/_dropout_ref.py.
  forward   kge_score_spo_dropout / kge_score_neg_dropout on the original tables return the bits kge_score_spo /
            kge_score_neg return on small tables that HOLD the masked rows, one row per occurrence (built with
            kge_embed_dropout): the mask is applied where a chunk is loaded, the arithmetic behind it is the undropped
            kernel's.
  backward  the two _dropout_bwd_accum entries against the float64 reference and derived bound of
            tests/_dropout_ref.py (bwd_reference): the closed forms of tests/_neg_bwd_ref.py on the masked rows, times the
            mask factor.  tests/test_dropout_ref_cpu.py shows on these inputs that a mask of the wrong call, a missing
            factor and a re-masked fixed row exceed the bound.  No tolerance here is measured; every case prints its
            largest err / bound (profiles/dropout_bound.txt is one such run)."""
import numpy as np
import pytest
import torch

import _dropout_ref as dr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 0x0BAD_5EED_1357_9BDF
DIMS = [2, 6, 36, 128, 130, 1024]
UNSUPPORTED = -2


def _t(x, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(DEV) if dtype is None else x.to(DEV, dtype)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _tables(name, d, E=23, R=5, l_norm=1.0, seed=0):
    from kge_amd import engine as eng
    rng = np.random.default_rng(1000 + d + seed)
    dr_ = d // 2 if name == "rotate" else d
    ent = rng.uniform(-1.5, 1.5, (E, d)).astype(np.float32)
    rel = rng.uniform(-1.5, 1.5, (R, dr_)).astype(np.float32)
    ent[3, :] = -ent[2, :]  # signs: a dropped negative element is -0
    return eng.Tables(name, _t(ent), _t(rel), l_norm=l_norm), ent, rel


# ---- the mask ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", [1, 33])
def test_embed_dropout_is_the_restatement_bit_for_bit(d, n):
    from kge_amd import engine as eng
    T, ent, rel = _tables("distmult", d)
    rng = np.random.default_rng(d + n)
    for table, tab, rows, p_ent, p_rel in (("ent", ent, 23, 0.3, 0.0), ("rel", rel, 5, 0.0, 0.6), ("ent", ent, 23, 0.5, 0.2),
                                           ("rel", rel, 5, 0.5, 0.2), ("ent", ent, 23, 0.0, 0.4)):
        idx = rng.integers(0, rows, n)
        if n > 1:
            idx[1] = idx[0]  # two occurrences of one row
        for role, occ0, call, itype in ((0, 0, 1, torch.int64), (2, 77, 3, torch.int32), (1, 2 ** 32 - n, 2 ** 32 + 5, torch.int64)):
            D = eng.Dropout(p_ent, p_rel, SEED, call)
            p = p_ent if table == "ent" else p_rel
            want = dr.embed(tab, idx, occ0, call, role, SEED, p)
            # a pitched output inside guard words
            buf = torch.full((n + 2, d + 7), float("nan"), device=DEV)
            out = buf[1:1 + n, 3:3 + d]
            wide = torch.zeros(2 * n + 1, dtype=itype, device=DEV)
            wide[1::2] = _t(idx, itype)
            got = eng.embed_dropout(T, table, wide[1::2], role, occ0, D, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert torch.equal(_bits(out), _bits(_t(want))), (table, role, occ0, p)
            guard = buf.clone()
            guard[1:1 + n, 3:3 + d] = float("nan")
            assert bool(torch.isnan(guard).all())
            if p == 0.0:
                assert torch.equal(_bits(out), _bits(_t(tab[idx])))
            elif n > 1 and d >= 36:
                assert not torch.equal(out[0], out[1])  # the same row, another occurrence: another mask


def test_declines_reach_the_front_end():
    from kge_amd import _lib, engine as eng
    T, _, _ = _tables("distmult", 8)
    ix = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        eng.embed_dropout(T, "ent", ix, 0, 2 ** 32 - 1, eng.Dropout(0.1, 0.0, 1, 1))  # occ reaches 2^32
    with pytest.raises(RuntimeError, match="unsupported"):
        eng.score_spo_dropout(T, ix, ix, ix, eng.Dropout(0.0, 0.0, 1, 1))
    Tb = eng.Tables("distmult", T.ent.bfloat16(), T.rel.bfloat16())
    with pytest.raises(RuntimeError, match="unsupported"):
        eng.score_spo_dropout(Tb, ix, ix, ix, eng.Dropout(0.1, 0.0, 1, 1))
    assert _lib.KGE_ERR_UNSUPPORTED == UNSUPPORTED


# ---- the forward bit contract ------------------------------------------------------------------------------------------
SCORERS = [("complex", 1.0), ("distmult", 1.0), ("transe", 1.0), ("transe", 2.0), ("rotate", 1.0)]


def _skip_width(name, d):
    return name in ("complex", "rotate") and (d // 2) % 2 == 1 and d > 2  # odd half-widths, as the existing tests


def _positives(n, E, R, rng):
    s, p, o = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    o[0] = s[0]  # s == o: two occurrences of one entity in one triple
    return s, p, o


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name,l_norm", SCORERS)
def test_score_spo_dropout_has_the_bits_of_score_spo_on_masked_rows(name, l_norm, d):
    from kge_amd import engine as eng
    if _skip_width(name, d):
        pytest.skip("odd half-width")
    T, ent, rel = _tables(name, d, l_norm=l_norm)
    rng = np.random.default_rng(7 * d)
    for n in (1, 33):
        for p_ent, p_rel in ((0.3, 0.2), (0.0, 0.5), (0.4, 0.0)):
            s, p, o = (_t(x) for x in _positives(n, 23, 5, rng))
            D = eng.Dropout(p_ent, p_rel, SEED + d, 11 + n)
            got = eng.score_spo_dropout(T, s, p, o, D)
            ent2 = torch.cat([eng.embed_dropout(T, "ent", s, 0, 0, D), eng.embed_dropout(T, "ent", o, 2, 0, D)])
            rel2 = eng.embed_dropout(T, "rel", p, 1, 0, D)
            T2 = eng.Tables(name, ent2, rel2, l_norm=l_norm)
            ar = torch.arange(n, device=DEV)
            want = eng.score_spo(T2, ar, ar, ar + n)
            assert torch.equal(_bits(got), _bits(want)), (n, p_ent, p_rel)
            if p_ent > 0 and d >= 36:
                assert not torch.equal(ent2[0], ent2[n])  # s == o, two masks
            other = eng.score_spo_dropout(T, s, p, o, eng.Dropout(p_ent, p_rel, SEED + d, 12 + n))
            if d >= 36:
                assert not torch.equal(got, other)  # another call, another mask


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name,l_norm", SCORERS)
def test_score_neg_dropout_has_the_bits_of_score_neg_on_masked_rows(name, l_norm, d):
    from kge_amd import engine as eng
    if _skip_width(name, d):
        pytest.skip("odd half-width")
    T, ent, rel = _tables(name, d, l_norm=l_norm)
    rng = np.random.default_rng(13 * d)
    for n in (1, 33):
        for K in (1, 5, 67):
            for slot in (0, 2):
                p_ent, p_rel = ((0.3, 0.2), (0.0, 0.5), (0.4, 0.0))[(n + K + slot) % 3]
                s, p, o = _positives(n, 23, 5, rng)
                neg = rng.integers(0, 23, (n, K))
                if K >= 5:
                    neg[:, 1] = neg[:, 0]  # a repeated entity inside a row
                    neg[0, 2] = s[0]
                wide = torch.zeros((n, K + 3), dtype=torch.int32 if slot == 0 else torch.int64, device=DEV)
                wide[:, 1:1 + K] = _t(neg)
                negd = wide[:, 1:1 + K]  # neg_ld > K
                sd, pd, od = _t(s), _t(p), _t(o)
                D = eng.Dropout(p_ent, p_rel, SEED + d, 100 + K)
                got = eng.score_neg_dropout(T, sd, pd, od, slot, negd, D)
                fixed, role_fixed = (od, 2) if slot == 0 else (sd, 0)
                ent2 = torch.cat([eng.embed_dropout(T, "ent", fixed, role_fixed, 0, D),
                                  eng.embed_dropout(T, "ent", _t(neg.reshape(-1)), slot, 0, D)])
                rel2 = eng.embed_dropout(T, "rel", pd, 1, 0, D)
                T2 = eng.Tables(name, ent2, rel2, l_norm=l_norm)
                ar = torch.arange(n, device=DEV)
                neg2 = n + torch.arange(n * K, device=DEV).view(n, K)
                want = eng.score_neg(T2, ar, ar, ar, slot, neg2)
                assert torch.equal(_bits(got), _bits(want)), (n, K, slot, p_ent, p_rel)
                if K >= 5 and p_ent > 0 and d >= 36:
                    assert not torch.equal(ent2[n], ent2[n + 1])  # one entity twice in a row: two masks


# ---- the backward --------------------------------------------------------------------------------------------------------
CASES = dr.bwd_cases()


def _pitched(x, extra):
    buf = torch.full((x.shape[0], x.shape[1] + extra), float("nan"), device=DEV)
    buf[:, :x.shape[1]] = x
    return buf, buf[:, :x.shape[1]]


@pytest.mark.parametrize("case", CASES, ids=dr.bwd_case_id)
def test_dropout_backward_within_the_derived_bound(case):
    from kge_amd import engine as eng
    c, slot, p_ent, p_rel, seed, call = case
    k = dr.make_bwd_case(case)
    (we, wr), (be, br), _ = dr.bwd_reference(k, p_ent, p_rel, seed, call)
    D = eng.Dropout(p_ent, p_rel, seed, call)
    T = eng.Tables(k["name"], _t(k["ent"]), _t(k["rel"]), l_norm=k["l_norm"])
    s, p, o, gout = _t(k["s"]), _t(k["p"]), _t(k["o"]), _t(k["gout"])
    pitched = bool(c.get("pitched"))
    ge_buf, ge = _pitched(_t(k["ge0"]), 5 if pitched else 0)
    gr_buf, gr = _pitched(_t(k["gr0"]), 3 if pitched else 0)
    need_scores = k["name"] in ("transe", "rotate") and k["l_norm"] != 1.0
    if k["kind"] == "neg":
        neg = _t(k["neg"], torch.int32 if slot == 2 else torch.int64)
        sc = eng.score_neg_dropout(T, s, p, o, slot, neg, D) if need_scores else None
        assert eng.score_neg_dropout_bwd_accum(T, s, p, o, slot, neg, gout, sc, ge, gr, D)
    else:
        sc = eng.score_spo_dropout(T, s, p, o, D) if need_scores else None
        assert eng.score_spo_dropout_bwd_accum(T, s, p, o, gout, sc, ge, gr, D)
    worst = []
    for got, want, bound, nm in ((ge, we, be, "grad_ent"), (gr, wr, br, "grad_rel")):
        g = got.double().cpu().numpy()
        assert np.isfinite(g).all(), nm
        err = np.abs(g - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bound, 0.0)
        worst.append(float(r.max()) if r.size else 0.0)
    print(f"dropout_bwd {dr.bwd_case_id(case)}: max err / bound  grad_ent {worst[0]:.4f}  grad_rel {worst[1]:.4f}")
    for buf, width in ((ge_buf, ge.shape[1]), (gr_buf, gr.shape[1])):
        assert bool(torch.isnan(buf[:, width:]).all())  # the pitch columns keep their bits
    assert max(worst) <= 1.0, worst
