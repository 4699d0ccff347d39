"""The float64 references of tests/_sharded_dense_ref.py, checked on the CPU before tests/test_gpu_sharded_dense_losses.py
holds the HIP kernels to them: the per-shard pieces, merged, are the whole-table losses of torch.nn.functional to
1e-12 (relative to max(1, |loss|): the bce rows are sums of a thousand terms), for both cut layouts of the GPU test;
the bf16-rounded query of the forward reference is the oracle's; and make_labels produces every edge it promises."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as ko

import _sharded_dense_ref as ref

LAYOUTS = [(1037, [0, 3, 68, 132, 1037]), (2000, [0, 1027, 2000])]
D, R, N = 16, 5, 37


def _case(seed, E):
    g = torch.Generator().manual_seed(seed)
    ent = (torch.randn(E, D, generator=g) * 0.5).bfloat16()
    rel = (torch.randn(R, D, generator=g) * 0.5).bfloat16()
    a, p = torch.randint(E, (N,), generator=g), torch.randint(R, (N,), generator=g)
    return ent, rel, a, p


def _close(got, want):
    err = (got - want).abs()
    assert bool((err <= 1e-12 * want.abs().clamp(min=1.0)).all()), float(err.max())


@pytest.mark.parametrize("E,cuts", LAYOUTS)
@pytest.mark.parametrize("model,direction", [("complex", "sp"), ("complex", "po"), ("distmult", "sp"), ("distmult", "po")])
def test_merged_shard_pieces_are_the_whole_table_losses(E, cuts, model, direction):
    ent, rel, a, p = _case(E + len(model), E)
    rng = np.random.default_rng(E)
    rowptr, col, info = ref.make_labels(rng, N, E, cuts)
    a_rows, p_rows = ent[a], rel[p]
    x = ref.scores64(model, direction, a_rows, p_rows, ent)
    shards = list(zip(cuts, cuts[1:]))
    xs = [ref.scores64(model, direction, a_rows, p_rows, ent[lo:hi]) for lo, hi in shards]
    assert torch.equal(torch.cat(xs, 1), x)
    # 1vsAll: labels at every border, the "elsewhere" label passed as -1 and as m
    lab = torch.from_numpy(np.resize(np.array(ref.boundary_ids(cuts) + [5, E // 2]), N))
    parts = []
    for k, ((lo, hi), xk) in enumerate(zip(shards, xs)):
        own = (lab >= lo) & (lab < hi)
        loc = torch.where(own, lab - lo, torch.full_like(lab, -1 if k % 2 else hi - lo))
        loss, lse = ref.ce64(xk, loc)
        assert torch.equal(torch.isnan(loss), ~own) and bool(torch.isfinite(lse).all())
        parts.append((loss, lse))
    loss, lse = ref.merge_ce(*zip(*parts))
    _close(loss, F.cross_entropy(x, lab, reduction="none"))
    _close(lse, torch.logsumexp(x, 1))
    # KvsAll kl: w = 1 / k and the -log k constant; rows without labels are 0
    y = ref.label_matrix(rowptr, col, 0, E)
    k = y.sum(1)
    assert torch.equal(k, torch.from_numpy(np.diff(rowptr)).double())
    w = torch.where(k > 0, 1.0 / k.clamp(min=1.0), torch.zeros_like(k))
    parts = [ref.kl_weighted64(xk, rowptr, col, lo, w) for (lo, hi), xk in zip(shards, xs)]
    assert torch.equal(sum(pk[2] for pk in parts), k)
    loss, lse = ref.merge_kl([pk[0] for pk in parts], [pk[1] for pk in parts])
    loss = torch.where(k > 0, loss - torch.log(k.clamp(min=1.0)), torch.zeros_like(loss))
    _close(loss, F.kl_div(torch.log_softmax(x, 1), F.normalize(y, p=1, dim=1), reduction="none").sum(1))
    # KvsAll bce with an offset
    parts = [ref.bce64(xk, rowptr, col, lo, -0.5) for (lo, hi), xk in zip(shards, xs)]
    assert torch.equal(sum(pk[1] for pk in parts), k)
    _close(ref.merge_bce([pk[0] for pk in parts]),
           F.binary_cross_entropy_with_logits(x - 0.5, y, reduction="none").sum(1))
    # ids that no shard owns change nothing
    rp2, cl2 = ref.with_extra_labels(rowptr, col, {0: [E], 1: [-1, E + 7], N - 1: [-5]})
    assert len(cl2) == len(col) + 4 and torch.equal(ref.label_matrix(rp2, cl2, 0, E), y)


@pytest.mark.parametrize("model,direction", [("complex", "sp"), ("complex", "po"), ("distmult", "sp"), ("distmult", "po")])
def test_gradient_references_are_autograd_of_the_torch_losses(model, direction):
    """ce_grads64 / kl_grads64 / bce_grads64 against autograd of torch.nn.functional's losses on the same float64 scores
    (the table rows as the only leaf there: g_ent is compared, 1e-12 of its largest entry)."""
    E, cuts = LAYOUTS[0]
    ent, rel, a, p = _case(3, E)
    rowptr, col, info = ref.make_labels(np.random.default_rng(1), N, E, cuts)
    a_rows, p_rows = ent[a], rel[p]
    g = (torch.rand(N, dtype=torch.float64) + 0.5) / N
    y = ref.label_matrix(rowptr, col, 0, E)
    k = y.sum(1)
    w = torch.where(k > 0, 1.0 / k.clamp(min=1.0), torch.zeros_like(k))
    lab = torch.from_numpy(np.resize(np.array(ref.boundary_ids(cuts)), N))

    def torch_grad(row_loss):
        e = ent.double().requires_grad_(True)
        (row_loss(ref.scores64(model, direction, a_rows, p_rows, e)) * g).sum().backward()
        return e.grad

    for got, want in (
            (ref.ce_grads64(model, direction, a_rows, p_rows, ent, lab, g),
             torch_grad(lambda x: F.cross_entropy(x, lab, reduction="none"))),
            # (rows without labels: w = 0, the reference's loss row is the lse alone -- the caller zeroes their g)
            (ref.kl_grads64(model, direction, a_rows, p_rows, ent, rowptr, col, w, g * (k > 0)),
             torch_grad(lambda x: F.kl_div(torch.log_softmax(x, 1), F.normalize(y, p=1, dim=1), reduction="none").sum(1))),
            (ref.bce_grads64(model, direction, a_rows, p_rows, ent, rowptr, col, -0.5, g),
             torch_grad(lambda x: F.binary_cross_entropy_with_logits(x - 0.5, y, reduction="none").sum(1)))):
        assert got[0].shape == a_rows.shape and got[1].shape == p_rows.shape
        assert float((got[2] - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("model", ["complex", "distmult"])
def test_bf16_rounded_query_is_the_oracles(model):
    """scores64(q_bf16=True) holds the query the way the project's bf16 semantics define it (oracle/kge_oracle.c: q in
    float32, rounded to bf16 once): the oracle's float32 scores differ by its accumulation alone, at most
    d * 2^-24 * sum_k |q_k t_k| -- a query that was NOT rounded is 2^-9 relative per element away, a hundred times that."""
    E = 300
    ent, rel, a, p = _case(7, E)
    O = ko.Tables(model, ko.f32_to_bf16(ent.float().numpy()), ko.f32_to_bf16(rel.float().numpy()), 1.0)
    for direction in ("sp", "po"):
        want = ko.score_sp(O, a.numpy(), p.numpy()) if direction == "sp" else ko.score_po(O, p.numpy(), a.numpy())
        got = ref.scores64(model, direction, ent[a], rel[p], ent, q_bf16=True)
        bound = D * 2.0 ** -24 * (ref.query64(model, direction, ent[a], rel[p], True).abs() @ ent.double().abs().t())
        err = (got - torch.from_numpy(want).double()).abs()
        assert bool((err <= bound).all()), (direction, float(err.max()), float(bound.min()))
        plain = ref.scores64(model, direction, ent[a], rel[p], ent)
        assert float((plain - got).abs().max()) > 10 * float(bound.max())   # (the rounding is visible at this bound)


@pytest.mark.parametrize("E,cuts", LAYOUTS)
@pytest.mark.parametrize("n", [ref.MIN_ROWS, 37, 160, 300])
def test_make_labels_produces_every_edge(E, cuts, n):
    rowptr, col, info = ref.make_labels(np.random.default_rng(n), n, E, cuts)
    assert rowptr.dtype == np.int64 and col.dtype == np.int64 and len(rowptr) == n + 1 and rowptr[-1] == len(col)
    rows = [col[rowptr[i]:rowptr[i + 1]] for i in range(n)]
    for r in rows:
        assert len(np.unique(r)) == len(r) and (r >= 0).all() and (r < E).all()
    nsh = len(cuts) - 1
    per = np.array([np.bincount(ref.shard_of(r, cuts), minlength=nsh) for r in rows])   # [n, shards] labels per shard
    bnd = ref.boundary_ids(cuts)
    assert set(bnd) == {0, E - 1} | {c - 1 for c in cuts[1:-1]} | {c for c in cuts[1:-1]}
    # the named rows are what they say
    assert len(rows[info["none"]]) == 0
    assert 64 < len(rows[info["many"]]) <= 80
    big = info["big_shard"]
    assert per[info["dense"], big] > 64 and per[info["dense"]].sum() == per[info["dense"], big]
    one = info["one_shard"]
    assert per[one].sum() > 0 and (per[one] > 0).sum() == 1
    assert (per[info["every_shard"]] > 0).all()
    for i in info["boundary"]:
        assert set(bnd) <= set(rows[i].tolist())
    for name, k in (("k4", 4), ("k5", 5), ("k8", 8)):
        assert per[info[name], big] == k and per[info[name]].sum() == k
    # ... and the properties hold for the CSR as a whole, wherever the rows are
    assert (per.sum(1) == 0).any() and (per > 64).any()
    assert all((per == k).any() for k in (4, 5, 8))
    assert ((per > 0).sum(1) == 1).any() and ((per > 0).sum(1) == nsh).any()
    for s in range(nsh):   # every shard has rows with all their labels elsewhere, and rows with none at all in it
        assert ((per[:, s] == 0) & (per.sum(1) > 0)).any()
    # first and last row carry labels or are an edge; the edge rows are spread over the batch
    assert per[info["elsewhere"], big] == 0 and per[info["elsewhere"]].sum() == 3
    named = [info[k] for k in ("none", "many", "dense", "every_shard", "k4", "k5", "k8", "elsewhere")] + info["boundary"]
    assert len(set(named)) == len(named) and min(named) == 0 and info["tail"] == n - 1
    # every boundary entity is a label of one to four rows
    cnt = np.bincount(col, minlength=E)
    assert (cnt[bnd] >= 1).all() and (cnt[bnd] <= 4).all(), cnt[bnd]
    # helpers
    rp1, cl1 = ref.take_rows(rowptr, col, [info["boundary"][0]])
    assert rp1.tolist() == [0, len(bnd)] and cl1.tolist() == bnd
    with pytest.raises(ValueError):
        ref.make_labels(np.random.default_rng(0), ref.MIN_ROWS - 1, E, cuts)
