"""tests/_wpenalty_ref.py against the reference's formula, without a GPU.

1. truth() -- unique / counts / len(indexes) in numpy float64 -- equals float64 torch autograd of the term as
   lookup_embedder.py:148-173 computes it (restated below line by line: unique with counts, the gather, abs for odd p,
   ** p times the counts, / len(indexes)), value and gradient, for lp p = 1, 2, 3 and n3 on a complex space, for a
   relation-style index vector and for the [n, 2] entity block of kge_model.py:616-618.
2. The float32 restatement the GPU test holds the kernels to follows that truth to float32 rounding.
3. Each way of getting the weighting wrong moves the value beyond the GPU test's bound and changes the bits of the
   stepped parameters, on the GPU test's own inputs (V, N, ids, tables of tests/test_gpu_wpenalty.py).

len() of the [n, 2] tensor the reference passes for the entity block is n, and that is what it divides by
(lookup_embedder.py:171): m = n is the truth here, and m = 2n (the flattened length) is one of the mutations."""
import numpy as np
import pytest
import torch

import _wpenalty_ref as wr
import test_gpu_wpenalty as g

KINDS = [("lp", 1), ("lp", 2), ("lp", 3), ("n3_complex", 3)]


def _reference_term(weight_t, indexes, kind, p, regularize_weight):
    """lookup_embedder.py:148-173 on a float64 table with autograd."""
    unique_indexes, counts = torch.unique(indexes, return_counts=True)
    parameters = weight_t[unique_indexes]
    if kind == "n3_complex":
        re, im = (t.contiguous() for t in parameters.chunk(2, dim=1))
        parameters = torch.sqrt(re ** 2 + im ** 2 + 1e-14)
    if (p % 2 == 1) and kind != "n3_complex":
        parameters = torch.abs(parameters)
    return (regularize_weight / p * (parameters ** p * counts.double().view(-1, 1))).sum() / len(indexes)


def _inputs(block):
    rng = np.random.default_rng(91)
    table = rng.standard_normal((g.V, 8))
    if block:
        ids = np.stack([g._ids(rng), g._ids(rng)], axis=1)
    else:
        ids = g._ids(rng)
    return table, ids


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("kind,p", KINDS)
def test_truth_equals_autograd_of_the_reference_formula(kind, p, block):
    table, ids = _inputs(block)
    w = torch.tensor(table, dtype=torch.float64, requires_grad=True)
    value = _reference_term(w, torch.from_numpy(ids), kind, p, g.WEIGHT)
    value.backward()
    v, grad = wr.truth(table, ids, kind, p, g.WEIGHT)
    assert abs(v - float(value)) <= 1e-13 * abs(float(value))
    assert np.allclose(grad, w.grad.numpy(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("kind,p", KINDS)
def test_float32_restatement_follows_the_truth(kind, p, block):
    table, ids = _inputs(block)
    t32 = table.astype(np.float32)
    m = len(ids)
    c = wr.counts_of(ids, g.V)
    pg, add = wr.penalty_gradient(t32, c, m, kind, p, g.WEIGHT)
    _v, grad = wr.truth(t32.astype(np.float64), ids, kind, p, g.WEIGHT)
    assert np.array_equal(add, c != 0) and not grad[~add].any()
    assert np.allclose(pg[add], grad[add], rtol=2e-6, atol=1e-9)   # a handful of float32 roundings
    v32 = g.WEIGHT / (3 if kind == "n3_complex" else p) / m * wr.value_sum64(t32, c, kind, p)
    assert abs(v32 - _v) <= 1e-12 * abs(_v)


def _mutations(ids_block):
    """name -> (counts, m, weight factor) as a wrong implementation would hand them to the kernel."""
    n = len(ids_block)
    true_c = wr.counts_of(ids_block, g.V)
    return {
        "unweighted factor": (np.full(g.V, n, np.uint32), n, 1.0),
        "1/m dropped": (true_c, 1, 1.0),
        "m = 2n (the flattened length) for the entity block": (true_c, 2 * n, 1.0),
        "a count of 1 per unique row": ((true_c != 0).astype(np.uint32), n, 1.0),
        "the doubled entity term": (true_c, n, 2.0),
    }


@pytest.mark.parametrize("kind,p", KINDS)
def test_every_mutation_exceeds_the_gpu_tests_bound(kind, p):
    rng = np.random.default_rng(11 + 8 + p)  # test_dense_adagrad's generator at dim 8
    ids = g._ids(rng)
    table, grad, (s,) = g._tables(rng, 8, 1)
    block = np.stack([ids, g._ids(rng)], axis=1)   # the entity block: N rows of (s, o)
    c, m = wr.counts_of(block, g.V), len(block)
    pn, sn, _ = wr.adagrad_dense(table, grad, s, c, m, kind, p, g.WEIGHT, g.MINUS_CLR, 0.0, g.EPS)
    pp = 3 if kind == "n3_complex" else p
    v_true = g.WEIGHT / pp / m * wr.value_sum64(table, c, kind, p)
    bound = g.WEIGHT / pp / m * wr.value_bound(table, c, kind, p, 1)
    for name, (mc, mm, wf) in _mutations(block).items():
        pm, _sm, _ = wr.adagrad_dense(table, grad, s, mc, mm, kind, p, wf * g.WEIGHT, g.MINUS_CLR, 0.0, g.EPS)
        assert not np.array_equal(pm.view(np.int32), pn.view(np.int32)), name
        v_mut = wf * g.WEIGHT / pp / mm * wr.value_sum64(table, mc, kind, p)
        assert abs(v_mut - v_true) > 100 * bound, (name, v_mut, v_true, bound)
