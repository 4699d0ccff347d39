"""kge_amd.optim.SparseAdam with touched rows under kge_amd.model on the MI355X, against torch.optim.SparseAdam on
`sparse=True` embeddings on the CPU: E = 300, R = 7, d = 16, n = 8, 4 negatives per slot, three steps.

The loss is linear in the scores with fixed weights, loss = sum w_pos score_spo + sum w_s score_neg(slot s) +
sum w_o score_neg(slot o): the gradient each score receives is its weight, exactly, on either side, so the only places
the two runs can part are the sums of the table gradients (float atomics on the GPU, index_add on the CPU) and the
optimizer's own roundings.  Bit equality is therefore not claimed; the bound is derived, per element, as follows.

A float64 run of the same three steps (gradients summed by hand in float64, tests/_sparse_adam_ref.step_touched_f64) is
the centre.  Either float32 run's gradient of a table element is a sum of K terms (K = the number of triples the row
takes part in, in that role):
  distmult  w a b (a, b the other two rows' elements): two roundings per term, K - 1 per sum in ANY order, so
            (K + 1) u sum |w a b| to first order -- taken as gamma = (K + 2) u / (1 - (K + 2) u) times sum |w a b| --, plus
            what the inputs' own distance to the float64 run moves the terms: sum |w| (|a| db + |b| da + da db);
  transe    -+ w sign(s + p - o) (l_norm 1): the terms are +-w exactly, so only the sum rounds: gamma sum |w|; the
            inputs' distance changes nothing as long as no sign flips, which the test ASSERTS on the float64 run:
            |s + p - o| > ds + dp + do + 4 u (|s| + |p| + |o|) for every element of every triple.
With that dg, _sparse_adam_ref.error_step carries bounds on moments and parameter through the step (its docstring derives
every line).  The two float32 runs are each within the bounds of the float64 run: they differ by at most twice them.
The largest |GPU - CPU| / (2 bound) seen is printed (profiles/sparse_adam_bound.txt keeps a run's lines).

Also here: the row sets that moved are identical, the relation table moves in the batch's p rows only, and a captured
step (kge_amd.train_graph.GraphedStep) replayed three times equals eager steps bit for bit -- on score_spo-only batches
whose s and o ids are unique and whose p ids occur at most twice (R = 7 < n = 8): a sum of two float atomics onto zero is
the same in either order, so no atomic ordering enters."""
import numpy as np
import pytest
import torch

import _sparse_adam_ref as sar
import _touched_ref as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, R, D, N, K = 300, 7, 16, 8, 4
LR, BETAS, EPS = 0.01, (0.9, 0.999), 1e-8
U = sar.U32


def _batches(seed, steps=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        out.append(dict(s=torch.randint(0, E, (N,), generator=g), p=torch.randint(0, R - 1, (N,), generator=g),
                        o=torch.randint(0, E, (N,), generator=g), neg_s=torch.randint(0, E, (N, K), generator=g),
                        neg_o=torch.randint(0, E, (N, K), generator=g), w_pos=torch.randn(N, generator=g),
                        w_s=torch.randn(N, K, generator=g), w_o=torch.randn(N, K, generator=g)))
    return out  # (relation R - 1 is never in a batch)


def _expanded(b):
    """Every scored triple of a batch with its weight: the positives, then each slot's corrupted triples."""
    s, p, o = b["s"], b["p"], b["o"]
    rep = lambda x: x.repeat_interleave(K)
    S = torch.cat([s, b["neg_s"].reshape(-1), rep(s)])
    P = torch.cat([p, rep(p), rep(p)])
    O = torch.cat([o, rep(o), b["neg_o"].reshape(-1)])
    W = torch.cat([b["w_pos"], b["w_s"].reshape(-1), b["w_o"].reshape(-1)])
    return S.numpy(), P.numpy(), O.numpy(), W.numpy().astype(np.float64)


def _cpu_score(name, ent, rel, s, p, o):
    se, pe, oe = ent(s), rel(p), ent(o)
    return (se * pe * oe).sum(-1) if name == "distmult" else -(se + pe - oe).abs().sum(-1)


def _gradients_f64(name, ent, rel, d_ent, d_rel, b):
    """The float64 run's table gradients, summed by hand, and the bound dg on either float32 run's distance to them
    (module docstring) -> (g_ent, g_rel, dg_ent, dg_rel, entity rows, relation rows)."""
    S, P, O, W = _expanded(b)
    g_ent, g_rel = np.zeros_like(ent), np.zeros_like(rel)
    a_ent, a_rel = np.zeros_like(ent), np.zeros_like(rel)      # sum |term|
    x_ent, x_rel = np.zeros_like(ent), np.zeros_like(rel)      # what the inputs' distance moves
    k_ent, k_rel = np.zeros(E), np.zeros(R)
    aw = np.abs(W)[:, None]
    se, pe, oe, ds, dp, do = ent[S], rel[P], ent[O], d_ent[S], d_rel[P], d_ent[O]
    if name == "distmult":
        prod = lambda a, b_: W[:, None] * a * b_
        moved = lambda a, da, b_, db: aw * (np.abs(a) * db + np.abs(b_) * da + da * db)
        parts = ((g_ent, a_ent, x_ent, k_ent, S, prod(pe, oe), moved(pe, dp, oe, do)),
                 (g_ent, a_ent, x_ent, k_ent, O, prod(se, pe), moved(se, ds, pe, dp)),
                 (g_rel, a_rel, x_rel, k_rel, P, prod(se, oe), moved(se, ds, oe, do)))
    else:
        x = se + pe - oe
        margin = ds + dp + do + 4 * U * (np.abs(se) + np.abs(pe) + np.abs(oe))
        assert (np.abs(x) > margin).all(), "an element of s + p - o too close to zero for the sign to be certain"
        sg = W[:, None] * np.sign(x)
        zero = np.zeros_like(sg)
        parts = ((g_ent, a_ent, x_ent, k_ent, S, -sg, zero), (g_ent, a_ent, x_ent, k_ent, O, sg, zero),
                 (g_rel, a_rel, x_rel, k_rel, P, -sg, zero))
    for g, a, xx, k, idx, term, mv in parts:
        np.add.at(g, idx, term)
        np.add.at(a, idx, np.abs(term))
        np.add.at(xx, idx, mv)
        np.add.at(k, idx, 1.0)
    gam = lambda k: ((k + 2) * U / (1 - (k + 2) * U))[:, None]
    return (g_ent, g_rel, x_ent + gam(k_ent) * a_ent, x_rel + gam(k_rel) * a_rel,
            sorted(set(S.tolist()) | set(O.tolist())), sorted(set(P.tolist())))


@pytest.mark.parametrize("name", ["distmult", "transe"])
def test_three_steps_against_torch_sparse_adam_on_sparse_embeddings(name):
    from kge_amd import model as kmodel, optim as kopt
    torch.manual_seed(3)
    m = kmodel.create(name, E, R, D, device=DEV)
    ent_w, rel_w = m.get_s_embedder().weight, m.get_p_embedder().weight
    init = [ent_w.detach().cpu().clone(), rel_w.detach().cpu().clone()]
    opt = kopt.SparseAdam(m.parameters(), lr=LR, betas=BETAS, eps=EPS)
    pe_, pr_ = opt.enable_touched_rows(ent_w), opt.enable_touched_rows(rel_w)
    m.set_touched_rows(pe_, pr_)
    # the CPU side: sparse=True embeddings, torch's optimizer
    ent = torch.nn.Embedding(E, D, sparse=True, _weight=init[0].clone())
    rel = torch.nn.Embedding(R, D, sparse=True, _weight=init[1].clone())
    ref = torch.optim.SparseAdam([ent.weight, rel.weight], lr=LR, betas=BETAS, eps=EPS)
    # the float64 centre and the running bounds
    c = [init[0].numpy().astype(np.float64), init[1].numpy().astype(np.float64)]
    cm, cv = [np.zeros_like(x) for x in c], [np.zeros_like(x) for x in c]
    dp, dm, dv = ([np.zeros_like(x) for x in c] for _ in range(3))
    worst = 0.0
    for t, b in enumerate(_batches(7), start=1):
        dev = {k: v.to(DEV) for k, v in b.items()}
        opt.zero_grad(set_to_none=True)
        loss = ((dev["w_pos"] * m.score_spo(dev["s"], dev["p"], dev["o"])).sum()
                + (dev["w_s"] * m.score_neg(dev["s"], dev["p"], dev["o"], 0, dev["neg_s"])).sum()
                + (dev["w_o"] * m.score_neg(dev["s"], dev["p"], dev["o"], 2, dev["neg_o"])).sum())
        loss.backward()
        assert ent_w.grad is None and rel_w.grad is None and pe_.pending and pr_.pending
        opt.step()
        ref.zero_grad(set_to_none=True)
        S, P, O, W = (torch.from_numpy(x) for x in _expanded(b))
        (W.float() * _cpu_score(name, ent, rel, S, P, O)).sum().backward()
        assert ent.weight.grad.is_sparse and rel.weight.grad.is_sparse
        ref.step()
        # the float64 run and the bounds
        g_e, g_r, dg_e, dg_r, rows_e, rows_r = _gradients_f64(name, c[0], c[1], dp[0], dp[1], b)
        for i, (g, dg, rows, n_rows) in enumerate(((g_e, dg_e, rows_e, E), (g_r, dg_r, rows_r, R))):
            bm = tr.mark(rows, n_rows)
            pn, _, mn, vn = sar.step_touched_f64(c[i], g, cm[i], cv[i], bm, t, LR, BETAS[0], BETAS[1], EPS)
            a, b_, e = sar.error_step(g[rows], dg[rows], cm[i][rows], dm[i][rows], cv[i][rows], dv[i][rows], pn[rows],
                                      dp[i][rows], t, LR, BETAS[0], BETAS[1], EPS)
            dm[i][rows], dv[i][rows], dp[i][rows] = a, b_, e
            c[i], cm[i], cv[i] = pn, mn, vn
        torch.cuda.synchronize()
        for i, (w, w_ref, what) in enumerate(((ent_w, ent.weight, "entity"), (rel_w, rel.weight, "relation"))):
            got, want = w.detach().cpu().numpy(), w_ref.detach().numpy()
            moved, moved_ref = (got != init[i].numpy()).any(1), (want != init[i].numpy()).any(1)
            assert np.array_equal(moved, moved_ref), (what, t, "the row sets that moved differ")
            st, st_ref = opt.state[w], ref.state[w_ref]
            for label, x, y, bound, centre in (
                    ("param", got, want, dp[i], c[i]),
                    ("exp_avg", st["exp_avg"].cpu().numpy(), st_ref["exp_avg"].numpy(), dm[i], cm[i]),
                    ("exp_avg_sq", st["exp_avg_sq"].cpu().numpy(), st_ref["exp_avg_sq"].numpy(), dv[i], cv[i])):
                err = np.abs(x.astype(np.float64) - y.astype(np.float64))
                ratio = float((err / np.where(bound > 0, 2 * bound, np.inf)).max())
                worst = max(worst, ratio)
                print(f"sparse_adam_bound {name} step {t} {what} {label}: max |gpu - cpu| {err.max():.3e} "
                      f"max bound {2 * bound.max():.3e} max ratio {ratio:.3f}")
                assert (err <= 2 * bound).all(), (what, label, t, float(err.max()))
                # either run against the float64 centre
                assert (np.abs(x - centre) <= bound).all() and (np.abs(y - centre) <= bound).all(), (what, label, t)
            assert st["step"] == st_ref["step"] == t == opt.device_step_count(w)
    print(f"sparse_adam_bound {name}: largest error / bound ratio {worst:.3f}")
    # the relation table moved in the batches' p rows only (relation R - 1 is in no batch); buffers are clean
    used = sorted({int(x) for b in _batches(7) for x in b["p"]})
    rel_now = rel_w.detach().cpu()
    for r in range(R):
        assert bool((rel_now[r] != init[1][r]).any()) == (r in used), r
    assert not pe_[0].any() and not pe_[1].any() and not pr_[0].any() and not pr_[1].any()
    assert sorted(map(id, opt.stepped_params())) == sorted(map(id, (ent_w, rel_w)))


def _spo_batches(seed, steps):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        ids = torch.randperm(E, generator=g)[:2 * N]
        p = torch.cat([torch.randperm(R, generator=g), torch.randint(0, R, (1,), generator=g)])  # each id at most twice
        out.append((torch.stack([ids[:N], p, ids[N:]], dim=1).to(DEV), torch.randn(N, generator=g).to(DEV)))
    return out


@pytest.mark.parametrize("name", ["distmult", "transe"])
def test_a_captured_step_replayed_three_times_equals_eager_steps_bit_for_bit(name):
    from kge_amd import model as kmodel, optim as kopt
    from kge_amd.train_graph import GraphedStep
    batches = _spo_batches(5, 4)
    runs = []
    for graphed in (False, True):
        torch.manual_seed(3)
        m = kmodel.create(name, E, R, D, device=DEV)
        ent_w, rel_w = m.get_s_embedder().weight, m.get_p_embedder().weight
        opt = kopt.SparseAdam(m.parameters(), lr=LR, betas=BETAS, eps=EPS)
        m.set_touched_rows(opt.enable_touched_rows(ent_w), opt.enable_touched_rows(rel_w))
        loss_fn = lambda tri, w: (w * m.score_spo(tri[:, 0], tri[:, 1], tri[:, 2])).sum()
        gs = GraphedStep(loss_fn, opt, warmup=1, enabled=graphed)
        for tri, w in batches:
            gs(tri, w)
        torch.cuda.synchronize()
        if graphed:
            assert gs.disabled_reason is None and gs.captures == 1 and gs.replays == 3, vars(gs)
        runs.append([(w.detach().clone(), opt.state[w]["exp_avg"].clone(), opt.state[w]["exp_avg_sq"].clone(),
                      opt.state[w]["clock"].clone(), opt.state[w]["step"]) for w in (ent_w, rel_w)])
    for eager, replayed in zip(*runs):
        for x, y in zip(eager[:3], replayed[:3]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(eager[3], replayed[3]) and eager[4] == replayed[4] == 4 == int(eager[3][0])
