"""float64 references of the dense-row losses of entity-sharded training (kge_ce_emb_* / kge_kl_weighted_emb_* /
kge_bce_emb_*), shard by shard and merged, in torch on the CPU (a helper module, not a test; nothing here touches a GPU).

A shard is the entity rows [lo, hi) of the table; `cuts` = [0, ..., E] lists the shard borders.  Scores are
x_ij = <q_i, ent_j> with q_i from the dense query rows (the formulas of tests/test_gpu_ce.py::test_kl_fwd_bwd):
    DistMult         q = a * r
    ComplEx, "sp"    q = a * r        (complex product; a = s)
    ComplEx, "po"    q = conj(r) * a  (a = o)
Per shard (what one rank's kernels return):
    ce           lse_shard,  lse_shard - x[label_local]                       (NaN: label outside [0, m))
    kl_weighted  lse_shard,  lse_shard - w_i sum_{labels of row i in shard} x
    bce          sum_{j in shard} softplus(x_ij + offset) - sum_{labels in shard} (x_ij + offset)
Merged over the shards, in float64 (the merges add no error of their own): lse = logsumexp of the shards' lse, label
terms and bce values summed.  Gradients: float64 autograd of sum_i g_i L_i over the WHOLE table w.r.t. the dense query
rows and the table rows, L_i one of
    lse - x[label],    lse - w_i sum_{labels} x - b_i sum_{all j} x,    the bce sum.
"""
import numpy as np
import torch


def query64(model, direction, a_rows, p_rows, q_bf16=False):
    """[n, d] float64 query vectors of the dense rows.  q_bf16: rounded the way the scoring kernels hold them (the
    project's bf16 semantics, oracle/kge_oracle.c: q evaluated in float32 -- products of bf16 values are exact there, so
    that is ONE rounding of the exact value -- then rounded to bf16, nearest even); not differentiable."""
    a, r = a_rows.double(), p_rows.double()
    h = a.shape[1] // 2
    if model == "distmult":
        q = a * r
    elif model == "complex":
        are, aim, rre, rim = a[:, :h], a[:, h:], r[:, :h], r[:, h:]
        if direction == "sp":
            q = torch.cat([are * rre - aim * rim, are * rim + aim * rre], dim=1)
        else:
            q = torch.cat([are * rre + aim * rim, aim * rre - are * rim], dim=1)
    else:
        raise ValueError(model)
    return q.float().bfloat16().double() if q_bf16 else q


def scores64(model, direction, a_rows, p_rows, ent, q_bf16=False):
    """[n, len(ent)] float64 scores of the dense query rows against the table rows `ent`."""
    return query64(model, direction, a_rows, p_rows, q_bf16) @ ent.double().t()


def label_matrix(rowptr, col, lo, m):
    """[n, m] float64 0/1: the labels of the CSR (global ids) inside [lo, lo + m); ids elsewhere (other shards, or
    outside the table altogether) are skipped."""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    n = len(rowptr) - 1
    y = torch.zeros(n, m, dtype=torch.float64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    c = col - lo
    ok = (c >= 0) & (c < m)
    y[torch.from_numpy(rows[ok]), torch.from_numpy(c[ok])] = 1.0
    return y


def ce64(x, label_local):
    """x [n, m] float64 scores of ONE shard, label_local [n] -> (loss, lse); loss NaN where the label is outside [0, m)."""
    m = x.shape[1]
    lab = torch.as_tensor(label_local).long()
    lse = torch.logsumexp(x, dim=1)
    ok = (lab >= 0) & (lab < m)
    true = x.gather(1, lab.clamp(0, m - 1).view(-1, 1)).view(-1)
    return torch.where(ok, lse - true, torch.full_like(lse, float("nan"))), lse


def kl_weighted64(x, rowptr, col, col_lo, w):
    """-> (loss, lse, k): lse_shard - w_i * (sum of row i's label scores inside the shard), the shard's lse, and the
    number of row i's labels inside the shard."""
    y = label_matrix(rowptr, col, col_lo, x.shape[1])
    lse = torch.logsumexp(x, dim=1)
    return lse - torch.as_tensor(w).double() * (x * y).sum(1), lse, y.sum(1)


def bce64(x, rowptr, col, col_lo, offset):
    """-> (loss, k): sum_{j in shard} softplus(x_ij + offset) - sum_{labels in shard} (x_ij + offset)."""
    y = label_matrix(rowptr, col, col_lo, x.shape[1])
    z = x + offset
    return torch.nn.functional.softplus(z).sum(1) - (z * y).sum(1), y.sum(1)


# ---- merges over the shards (float64) --------------------------------------------------------------------------------
def merge_lse(lses):
    return torch.logsumexp(torch.stack([torch.as_tensor(z).double() for z in lses]), dim=0)


def merge_ce(losses, lses):
    """The owner's label score is lse_shard - loss_shard; the other shards' loss rows are NaN."""
    lse = merge_lse(lses)
    true = torch.zeros_like(lse)
    for loss, z in zip(losses, lses):
        loss, z = torch.as_tensor(loss).double(), torch.as_tensor(z).double()
        true = true + torch.where(torch.isnan(loss), torch.zeros_like(z), z - loss)
    return lse - true, lse


def merge_kl(losses, lses):
    """lse_global - sum over the shards of w_i * (label scores in the shard) = lse_global - sum (lse_shard - loss_shard)."""
    lse = merge_lse(lses)
    terms = sum(torch.as_tensor(z).double() - torch.as_tensor(loss).double() for loss, z in zip(losses, lses))
    return lse - terms, lse


def merge_bce(losses):
    return sum(torch.as_tensor(loss).double() for loss in losses)


# ---- gradients (float64 autograd over the whole table) ----------------------------------------------------------------
def _grads(model, direction, a_rows, p_rows, ent, g, row_loss):
    a = a_rows.double().clone().requires_grad_(True)
    p = p_rows.double().clone().requires_grad_(True)
    e = ent.double().clone().requires_grad_(True)
    x = scores64(model, direction, a, p, e)
    (row_loss(x) * torch.as_tensor(g).double()).sum().backward()
    return a.grad, p.grad, e.grad


def ce_grads64(model, direction, a_rows, p_rows, ent, label, g):
    """(g_a [n, d], g_p [n, d], g_ent [E, d]) of sum_i g_i (lse_i - x[i, label_i])."""
    lab = torch.as_tensor(label).long()
    return _grads(model, direction, a_rows, p_rows, ent, g,
                  lambda x: torch.logsumexp(x, 1) - x.gather(1, lab.view(-1, 1)).view(-1))


def kl_grads64(model, direction, a_rows, p_rows, ent, rowptr, col, w, g, bias=None):
    """... of sum_i g_i (lse_i - w_i sum_{labels} x_ij - b_i sum_{all j} x_ij); b = 0 without label smoothing."""
    y = label_matrix(rowptr, col, 0, ent.shape[0])
    w = torch.as_tensor(w).double()
    b = torch.zeros_like(w) if bias is None else torch.as_tensor(bias).double()
    return _grads(model, direction, a_rows, p_rows, ent, g,
                  lambda x: torch.logsumexp(x, 1) - w * (x * y).sum(1) - b * x.sum(1))


def bce_grads64(model, direction, a_rows, p_rows, ent, rowptr, col, offset, g):
    y = label_matrix(rowptr, col, 0, ent.shape[0])
    return _grads(model, direction, a_rows, p_rows, ent, g,
                  lambda x: torch.nn.functional.softplus(x + offset).sum(1) - ((x + offset) * y).sum(1))


# ---- label generator --------------------------------------------------------------------------------------------------
MIN_ROWS = 11  # the rows make_labels needs for its edges


def boundary_ids(cuts):
    """0, E - 1 and both sides of every inner cut: the entity rows next to a shard border."""
    E = cuts[-1]
    ids = {0, E - 1}
    for c in cuts[1:-1]:
        ids |= {c - 1, c}
    return sorted(ids)


def shard_of(ids, cuts):
    return np.searchsorted(np.asarray(cuts), np.asarray(ids), side="right") - 1


def make_labels(rng, n, E, cuts):
    """(rowptr [n + 1], col [nnz], info): an int64 label CSR of n >= MIN_ROWS rows, global ids, unique (and sorted) per
    row.  Random rows (1..7 labels) and, spread evenly from row 0 to row n - 1 (info names them):
      "none"         a row without labels
      "many"         70 labels anywhere
      "dense"        66 labels inside the largest shard (bce/kl_sub_kernel stride the labels by 64), none elsewhere
      "one_shard"    5 labels, all inside the largest shard   (== "k5")
      "elsewhere"    3 labels, all inside the second largest shard: the largest has a row with labels, none of them its own
      "every_shard"  one label in every shard
      "boundary"     two rows that each hold ALL of boundary_ids(cuts)
      "k4", "k5", "k8"  exactly 4, 5, 8 labels inside the largest shard, none elsewhere (kl_label_sum takes four at a time)
    Only the two boundary rows -- and "every_shard", in a shard that has no other id -- hold a boundary id: each of them
    is a label of at most four rows, so one dropped label moves its gradient row by a quarter of its norm or more."""
    cuts = [int(c) for c in cuts]
    assert cuts[0] == 0 and cuts[-1] == E and all(b > a for a, b in zip(cuts, cuts[1:])), cuts
    if n < MIN_ROWS:
        raise ValueError(f"make_labels: {n} rows cannot hold the {MIN_ROWS} edge rows")
    bnd = boundary_ids(cuts)
    inner = np.setdiff1d(np.arange(E), bnd)            # what random labels are drawn from
    big = int(np.argmax(np.diff(cuts)))
    in_big = inner[(inner >= cuts[big]) & (inner < cuts[big + 1])]
    second = int(np.argsort(np.diff(cuts))[-2])
    in_second = inner[(inner >= cuts[second]) & (inner < cuts[second + 1])]
    if len(in_big) < 66 or len(inner) < 70 or len(in_second) < 3:
        raise ValueError("make_labels: the two largest shards are too small for the edge rows")
    pick = lambda pool, k: np.sort(rng.choice(pool, k, replace=False))
    every = []
    for lo, hi in zip(cuts, cuts[1:]):
        pool = inner[(inner >= lo) & (inner < hi)]
        every.append(int(rng.choice(pool if len(pool) else np.arange(lo, hi))))
    special = {
        "none": np.zeros(0, np.int64),
        "many": pick(inner, 70),
        "dense": pick(in_big, 66),
        "every_shard": np.sort(np.array(every)),
        "boundary0": np.array(bnd),
        "boundary1": np.union1d(bnd, pick(inner, 3)),
        "k4": pick(in_big, 4),
        "k5": pick(in_big, 5),
        "k8": pick(in_big, 8),
        "elsewhere": pick(in_second, 3),
        "tail": pick(in_big, 2),                       # the last row: labels, all in one shard
    }
    where = np.unique(np.round(np.linspace(0, n - 1, len(special))).astype(int))
    assert len(where) == len(special)
    rows = [pick(inner, int(rng.integers(1, 8))) for _ in range(n)]
    info = {}
    for (name, ids), i in zip(special.items(), where):
        rows[int(i)] = ids.astype(np.int64)
        info[name] = int(i)
    info["boundary"] = [info.pop("boundary0"), info.pop("boundary1")]
    info["one_shard"] = info["k5"]
    info["big_shard"] = big
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int64)
    return rowptr, col, info


def take_rows(rowptr, col, rows):
    """The CSR of the listed rows only."""
    parts = [col[rowptr[i]:rowptr[i + 1]] for i in rows]
    return (np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64),
            np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.int64))


def with_extra_labels(rowptr, col, extra):
    """The CSR with the ids extra[i] appended to row i (for ids no shard owns: negative, or >= E)."""
    n = len(rowptr) - 1
    parts = [np.concatenate([col[rowptr[i]:rowptr[i + 1]], np.asarray(extra.get(i, []), np.int64)]) for i in range(n)]
    return (np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64),
            np.concatenate(parts).astype(np.int64))
