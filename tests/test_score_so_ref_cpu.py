"""tests/_score_so_ref.py against independent statements (no GPU): its scores against the torch port of the reference
scorers on every (i, j), its gradients against torch float64 autograd through the reference's repeat composition
(kge_model.py:202-209), and the properties of the case list tests/test_gpu_score_so.py runs."""
import numpy as np
import pytest
import torch

import _score_so_ref as SO
import torch_port as tp


def _repeat_composition(name, l_norm, ent, rel, s, o, rels):
    """RelationalScorer.score_emb(..., "s_o"): repeat_interleave / repeat to [n m, d], then the spo form"""
    se, oe = ent[s], ent[o]
    pe = rel if rels is None else rel[rels]
    n, m = se.shape[0], pe.shape[0]
    return tp.score_emb(name, se.repeat_interleave(m, 0), pe.repeat((n, 1)), oe.repeat_interleave(m, 0), "spo",
                        l_norm).view(n, m)


@pytest.fixture(scope="module", params=SO.BWD_CASES, ids=SO.case_id)
def case(request):
    return SO.make_case(request.param)


def _t(x, dtype):
    return None if x is None else torch.from_numpy(np.asarray(x)).to(dtype)


def test_scores_match_the_torch_port_on_every_pair(case):
    k = case
    s, o, rels = (_t(k[x], torch.long) for x in ("s", "o", "rels"))
    ref = SO.scores(k["name"], k["l_norm"], k["ent"], k["rel"], k["s"], k["o"], k["rels"])
    assert ref.shape == (k["n"], k["m"])
    ent, rel = _t(k["ent"], torch.float32), _t(k["rel"], torch.float32)
    P = torch.arange(k["R"]) if rels is None else rels
    for j in range(k["m"]):  # the spo scores of column j, one call per column
        got = tp.score_spo(k["name"], ent, rel, s, P[j].expand(k["n"]), o, k["l_norm"]).numpy()
        scale = max(1.0, float(np.sqrt(np.mean(ref[:, j] ** 2))))
        np.testing.assert_allclose(got, ref[:, j], atol=1e-5 * scale, rtol=1e-4)  # test_oracle_vs_reference.py
        bound = SO.scores_bound(k["name"], k["l_norm"], k["ent"], k["rel"], k["s"], k["o"], k["rels"])[:, j]
        assert (np.abs(got.astype(np.float64) - ref[:, j]) <= bound).all()


def test_gradients_match_float64_autograd_through_the_repeats(case):
    k = case
    s, o, rels = (_t(k[x], torch.long) for x in ("s", "o", "rels"))
    ent = _t(k["ent"], torch.float64).requires_grad_()
    rel = _t(k["rel"], torch.float64).requires_grad_()
    sc = _repeat_composition(k["name"], k["l_norm"], ent, rel, s, o, rels)
    np.testing.assert_allclose(sc.detach().numpy(), SO.scores(k["name"], k["l_norm"], k["ent"], k["rel"], k["s"],
                                                              k["o"], k["rels"]), rtol=1e-12, atol=1e-12)
    (sc * _t(k["gout"], torch.float64)).sum().backward()
    ge, gr = SO.bwd_accum(*SO.ref_args(k))
    np.testing.assert_allclose(ge - k["ge0"], ent.grad.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(gr - k["gr0"], rel.grad.numpy(), rtol=1e-9, atol=1e-9)
    be, br = SO.bwd_accum_bound(*SO.ref_args(k))
    me, mr = SO.owned_rows(k["s"], k["o"], k["rels"], k["E"], k["R"])
    assert (be[me] > 0).all() and (br[mr] > 0).all() and not be[~me].any() and not br[~mr].any()
    assert (ge[~me] == k["ge0"][~me]).all() and (gr[~mr] == k["gr0"][~mr]).all()


def test_the_case_list_covers_what_the_kernels_branch_on():
    seen = set()
    for c in SO.BWD_CASES:
        k = SO.make_case(c)
        seen.add((c["name"], c["d"], c["n"], c["m"], c["listed"]))
        me, mr = SO.owned_rows(k["s"], k["o"], k["rels"], k["E"], k["R"])
        assert (~me).sum() >= 3 and (c["listed"] is False or (~mr).sum() >= 3)
        if c["n"] >= 2:
            assert k["s"][0] == k["o"][0]                                     # s[i] == o[i]
            assert (k["s"][-1], k["o"][-1]) == (k["s"][1], k["o"][1])         # a repeated pair
        if c["listed"] and c["m"] >= 2:
            assert k["rels"][-1] == k["rels"][0] and (np.diff(k["rels"]) < 0).any()  # repeated, unsorted
    for name in SO.NAMES:
        for d in (16, SO.scalar_dim(name), 72):
            for n, m in ((1, 5), (33, 5), (1, 33), (33, 33)):
                assert (name, d, n, m, True) in seen and (name, d, n, m, False) in seen
    assert {(c["name"], c["l_norm"]) for c in SO.BWD_CASES} >= {("transe", 2.0), ("transe", 3.0), ("rotate", 2.0),
                                                                ("rotate", 3.0)}
