"""The autograd nodes of kge_amd.model with the touched-row pair on the MI355X.

_ScoreNegBlocks, _ScoreSPO and _ScoreNeg take an optional (grad, bitmap) pair of kge_amd.optim.Adagrad.enable_touched_rows:
the backward then marks s, o and the negative blocks it differentiates, runs the accumulate kernels on the persistent
`grad` in place of a fresh zeros_like(ent), and returns None for the entity table.

DistMult, ComplEx and TransE (l_norm 1) run on INTEGER tables and upstream gradients, |x| <= 4: every product and every
partial sum of the backward is then an integer below 2^24 (checked on the CPU below), exact in float32 whatever the
order of the float atomics -- so the persistent buffer must equal the dense node's gradient BIT FOR BIT, and one
Adagrad.step() each way must leave bit-equal parameters and accumulators.  RotatE (cos / sin of the phases: no integer
form) runs on random tables against the float64 closed forms and elementwise bounds of tests/_neg_bwd_ref.py."""
import numpy as np
import pytest
import torch

import _neg_bwd_ref as nb
import _touched_ref as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, R, D, N, K = 70, 5, 8, 9, 7
INT_MODELS = [("distmult", 1.0), ("complex", 1.0), ("transe", 1.0)]


def _case(name, integers=True, seed=0):
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    dr = D // 2 if name == "rotate" else D
    if integers:
        ent = rng.integers(-4, 5, (E, D)).astype(np.float32)
        rel = rng.integers(-4, 5, (R, dr)).astype(np.float32)
        g = [rng.integers(-4, 5, shape).astype(np.float32) for shape in ((N,), (N,), (N, K), (N, K))]
    else:
        ent = rng.standard_normal((E, D)).astype(np.float32)
        rel = rng.uniform(-np.pi, np.pi, (R, dr)).astype(np.float32)
        g = [rng.standard_normal(shape).astype(np.float32) for shape in ((N,), (N,), (N, K), (N, K))]
    # ids with repeats: a small pool for the positives, negatives that hit positives and each other
    s = rng.integers(0, 12, N)
    o = rng.integers(6, 20, N)
    p = rng.integers(0, R, N)
    neg_s = rng.integers(0, 30, (N, K))
    neg_o = rng.integers(10, E, (N, K))
    neg_o[:, 0] = neg_o[0, 0]
    return dict(name=name, ent=ent, rel=rel, s=s, p=p, o=o, neg_s=neg_s, neg_o=neg_o, g_pos_s=g[0], g_pos_o=g[1],
                g_s=g[2], g_o=g[3])


def _dev(c):
    t = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    tri = t(np.stack([c["s"], c["p"], c["o"]], 1))   # s, p, o as the stride-3 columns the jobs hand over
    return dict(tri=tri, s=tri[:, 0], p=tri[:, 1], o=tri[:, 2], neg_s=t(c["neg_s"]), neg_o=t(c["neg_o"]),
                g_pos_s=t(c["g_pos_s"]), g_pos_o=t(c["g_pos_o"]), g_s=t(c["g_s"]), g_o=t(c["g_o"]))


def _params(c):
    ent = torch.nn.Parameter(torch.from_numpy(c["ent"]).to(DEV))
    rel = torch.nn.Parameter(torch.from_numpy(c["rel"]).to(DEV))
    return ent, rel


def _blocks_backward(c, d, l_norm, ent, rel, pair):
    from kge_amd.model import _ScoreNegBlocks
    pos, sc_s, sc_o = _ScoreNegBlocks.apply(c["name"], l_norm, ent, rel, d["s"], d["p"], d["o"], d["neg_s"], d["neg_o"],
                                            pair)
    # (the positives' gradient arrives once per slot in the job: here their sum)
    torch.autograd.backward([pos, sc_s, sc_o], [d["g_pos_s"] + d["g_pos_o"], d["g_s"], d["g_o"]])


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _want_bitmap(c):
    return tr.mark(np.concatenate([c["s"], c["o"], c["neg_s"].reshape(-1), c["neg_o"].reshape(-1)]), E)


def test_the_integer_cases_are_exact_in_float32():
    """CPU arithmetic only: |table| <= 4 and |gout| <= 4 make every term of every gradient element an integer of
    magnitude <= 2 * 4 * 4 * |g| (ComplEx: two products per term; DistMult one; TransE l1: |g|), so ANY partial sum of
    the terms of the whole call is bounded by sum |g| * 32 over all scored triples -- below 2^24, where float32 holds
    every integer: the order of the atomics cannot matter."""
    for name, _ in INT_MODELS:
        c = _case(name)
        assert np.abs(c["ent"]).max() <= 4 and np.abs(c["rel"]).max() <= 4
        assert all(np.array_equal(c[k], np.round(c[k])) for k in ("ent", "rel", "g_pos_s", "g_pos_o", "g_s", "g_o"))
        total = sum(float(np.abs(c[k]).sum()) for k in ("g_pos_s", "g_pos_o", "g_s", "g_o"))
        assert total * 2 * 4 * 4 < 2 ** 24
        # and the closed forms in float64 give integers (what the float32 kernels must then hit exactly)
        S = np.concatenate([c["s"], c["neg_s"].reshape(-1), np.repeat(c["s"], K)])
        P = np.concatenate([c["p"], np.repeat(c["p"], K), np.repeat(c["p"], K)])
        O = np.concatenate([c["o"], np.repeat(c["o"], K), c["neg_o"].reshape(-1)])
        g = np.concatenate([c["g_pos_s"] + c["g_pos_o"], c["g_s"].reshape(-1), c["g_o"].reshape(-1)])
        ge, gr = nb.spo_bwd_accum(name, 1.0, c["ent"].astype(np.float64), c["rel"].astype(np.float64), S, P, O, g,
                                  np.zeros((E, D)), np.zeros(c["rel"].shape))
        assert np.array_equal(ge, np.round(ge)) and np.array_equal(gr, np.round(gr))
        assert np.abs(ge).max() < 2 ** 24 and np.abs(gr).max() < 2 ** 24


@pytest.mark.parametrize("name,l_norm", INT_MODELS)
def test_blocks_node_fills_the_persistent_buffer_with_the_dense_gradient_bits(name, l_norm):
    from kge_amd.optim import Adagrad
    c = _case(name)
    d = _dev(c)
    # the dense way
    entA, relA = _params(c)
    optA = Adagrad([entA, relA], lr=0.1)
    _blocks_backward(c, d, l_norm, entA, relA, None)
    assert entA.grad is not None and relA.grad is not None
    # the touched-row way
    entB, relB = _params(c)
    optB = Adagrad([entB, relB], lr=0.1)
    assert optB.touched_rows(entB) is None
    pair = optB.enable_touched_rows(entB)
    assert optB.touched_rows(entB) is pair and optB.enable_touched_rows(entB) is pair   # allocated once
    grad, bitmap = pair
    assert tuple(grad.shape) == (E, D) and not grad.any() and not bitmap.any()
    _blocks_backward(c, d, l_norm, entB, relB, pair)
    assert entB.grad is None, "the entity table's gradient must stay in the persistent buffer"
    assert torch.equal(_bits(grad), _bits(entA.grad)), "persistent buffer != the dense node's gradient"
    assert torch.equal(_bits(relB.grad), _bits(relA.grad))
    assert np.array_equal(bitmap.cpu().numpy().view(np.uint32), _want_bitmap(c))
    # the float64 closed forms agree with both (integers: exactly)
    S = np.concatenate([c["s"], c["neg_s"].reshape(-1), np.repeat(c["s"], K)])
    P = np.concatenate([c["p"], np.repeat(c["p"], K), np.repeat(c["p"], K)])
    O = np.concatenate([c["o"], np.repeat(c["o"], K), c["neg_o"].reshape(-1)])
    g = np.concatenate([c["g_pos_s"] + c["g_pos_o"], c["g_s"].reshape(-1), c["g_o"].reshape(-1)])
    ge, _ = nb.spo_bwd_accum(name, l_norm, c["ent"].astype(np.float64), c["rel"].astype(np.float64), S, P, O, g,
                             np.zeros((E, D)), np.zeros(c["rel"].shape))
    assert np.array_equal(grad.cpu().numpy().astype(np.float64), ge)
    # one step each way: bit-equal parameters and accumulators, buffer and bitmap zero again, the step counted
    optA.step()
    optB.step()
    assert torch.equal(_bits(entB), _bits(entA)) and torch.equal(_bits(relB), _bits(relA))
    assert torch.equal(_bits(optB.state[entB]["sum"]), _bits(optA.state[entA]["sum"]))
    assert torch.equal(_bits(optB.state[relB]["sum"]), _bits(optA.state[relA]["sum"]))
    assert not _bits(grad).any() and not bitmap.any()
    assert float(optB.state[entB]["step"]) == 1.0 and float(optA.state[entA]["step"]) == 1.0
    assert [q is entB or q is relB for q in optB.stepped_params()] == [True, True]
    assert not torch.equal(_bits(entB), _bits(torch.from_numpy(c["ent"]).to(DEV))), "the step moved nothing"


@pytest.mark.parametrize("name,l_norm", INT_MODELS)
def test_separate_nodes_in_the_eager_jobs_order_give_the_blocks_buffer(name, l_norm):
    """TrainingJobNegativeSampling._process_subbatch (train_negative_sampling.py:120-164) per slot: score_spo, the
    slot's score_neg, the loss, backward -- _ScoreSPO + _ScoreNeg for the subject slot, then for the object slot."""
    from kge_amd.model import _ScoreNeg, _ScoreSPO
    from kge_amd.optim import Adagrad
    c = _case(name)
    d = _dev(c)
    ent1, rel1 = _params(c)
    pair1 = Adagrad([ent1, rel1], lr=0.1).enable_touched_rows(ent1)
    _blocks_backward(c, d, l_norm, ent1, rel1, pair1)
    ent2, rel2 = _params(c)
    pair2 = Adagrad([ent2, rel2], lr=0.1).enable_touched_rows(ent2)
    for slot, neg, gp, gn in ((0, d["neg_s"], d["g_pos_s"], d["g_s"]), (2, d["neg_o"], d["g_pos_o"], d["g_o"])):
        pos = _ScoreSPO.apply(name, l_norm, ent2, rel2, d["s"], d["p"], d["o"], pair2)
        sc = _ScoreNeg.apply(name, l_norm, ent2, rel2, d["s"], d["p"], d["o"], slot, neg, pair2)
        torch.autograd.backward([pos, sc], [gp, gn])
    assert ent1.grad is None and ent2.grad is None
    assert torch.equal(_bits(pair2[0]), _bits(pair1[0]))
    assert torch.equal(pair2[1], pair1[1]) and pair1[1].any()
    assert torch.equal(_bits(rel2.grad), _bits(rel1.grad))
    # the same two nodes WITHOUT the pair still return the dense gradient (existing behaviour, unchanged)
    ent3, rel3 = _params(c)
    pos = _ScoreSPO.apply(name, l_norm, ent3, rel3, d["s"], d["p"], d["o"])
    sc = _ScoreNeg.apply(name, l_norm, ent3, rel3, d["s"], d["p"], d["o"], 0, d["neg_s"])
    torch.autograd.backward([pos, sc], [d["g_pos_s"], d["g_s"]])
    assert ent3.grad is not None and ent3.grad.shape == ent3.shape


def test_rotate_buffer_within_the_float64_bounds():
    c = _case("rotate", integers=False)
    d = _dev(c)
    from kge_amd.optim import Adagrad
    ent, rel = _params(c)
    grad, bitmap = pair = Adagrad([ent, rel], lr=0.1).enable_touched_rows(ent)
    _blocks_backward(c, d, 1.0, ent, rel, pair)
    assert ent.grad is None
    S = np.concatenate([c["s"], c["neg_s"].reshape(-1), np.repeat(c["s"], K)])
    P = np.concatenate([c["p"], np.repeat(c["p"], K), np.repeat(c["p"], K)])
    O = np.concatenate([c["o"], np.repeat(c["o"], K), c["neg_o"].reshape(-1)])
    g = np.concatenate([c["g_pos_s"] + c["g_pos_o"], c["g_s"].reshape(-1), c["g_o"].reshape(-1)])
    (ge, gr), (be, br) = nb._accum("rotate", 1.0, c["ent"].astype(np.float64), c["rel"].astype(np.float64), S, P, O, g,
                                   np.zeros((E, D)), np.zeros(c["rel"].shape), None, True)
    err_e = np.abs(grad.cpu().numpy().astype(np.float64) - ge)
    err_r = np.abs(rel.grad.cpu().numpy().astype(np.float64) - gr)
    print(f"rotate: max err / bound, entity {np.max(err_e / np.maximum(be, 1e-300)):.3f} relation "
          f"{np.max(err_r / np.maximum(br, 1e-300)):.3f}")
    assert (err_e <= be).all(), float((err_e - be).max())
    assert (err_r <= br).all(), float((err_r - br).max())
    assert np.array_equal(bitmap.cpu().numpy().view(np.uint32), _want_bitmap(c))
    # rows nothing was added to: bound 0, and the buffer's bits are zero there
    untouched = np.setdiff1d(np.arange(E), tr.marked_rows(_want_bitmap(c), E))
    assert untouched.size and not grad[torch.from_numpy(untouched).to(DEV)].view(torch.int32).any()


def test_step_refuses_a_dense_gradient_and_a_fused_penalty_on_a_touched_parameter():
    from kge_amd.optim import Adagrad
    c = _case("distmult")
    ent, rel = _params(c)
    opt = Adagrad([ent, rel], lr=0.1)
    opt.enable_touched_rows(ent)
    ent.grad = torch.zeros_like(ent)
    with pytest.raises(RuntimeError, match="dense gradient"):
        opt.step()
    ent.grad = None
    opt.set_penalty(ent, "lp", 2, 1e-3)
    with pytest.raises(RuntimeError, match="penalty"):
        opt.step()
    opt.set_penalty(ent, None, 0, 0.0)
    opt.step()                                           # nothing marked: nothing moves, the step is counted
    assert torch.equal(ent.detach(), torch.from_numpy(c["ent"]).to(DEV)) and float(opt.state[ent]["step"]) == 1.0
    with pytest.raises(ValueError):
        Adagrad([ent], lr=0.1, weight_decay=0.01).enable_touched_rows(ent)
    half = torch.nn.Parameter(ent.detach().half())
    with pytest.raises(ValueError):
        Adagrad([half], lr=0.1).enable_touched_rows(half)
    vec = torch.nn.Parameter(torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        Adagrad([vec], lr=0.1).enable_touched_rows(vec)
