#!/usr/bin/env python3
"""What kge_amd.optim.SparseAdam on touched rows (kge_sparse_adam_step_touched) does to the
negative-sampling training step: DistMult, n = 512 triples per batch, K = 256 uniform negatives per slot, both slots,
d = 128, bce loss on every slot's [n, 1 + K] block, for an entity table of 14,541 rows (the FB15k-237 shape) and of
4,594,485 rows (the Wikidata5M shape).  Three arms per table size, all built from this tree:
  sparse_touched  kge_amd.model + kge_amd.optim.SparseAdam, both tables through their bitmaps; captured step
  adam_dense      kge_amd.model + kge_amd.optim.Adam(device_step=True): dense gradients, kge_adam_step_multi sweeps
                  both tables; captured step.  (A different optimizer: its momentum moves every row.)
  torch_sparse    nn.Embedding(sparse=True) tables, the scores as the torch op sequence (gather, multiply, sum),
                  torch.optim.SparseAdam; eager -- its coalesce() reads a size on the host, it cannot be captured
ms per step: the arms' windows ALTERNATE (one window of `--steps` steps of each arm in turn, `--windows` rounds), HIP
events around each window, median and min..max per arm.  The last loss of each arm is printed as a check.

    python tools/sparse_adam_probe.py [--windows 9] [--steps 40] [--entities 14541,4594485] [--out FILE]
Writes its table to profiles/sparse_adam_probe.txt (or --out)."""
import argparse
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kge_amd import model as km, optim as kopt  # noqa: E402
from kge_amd.train_graph import GraphedStep  # noqa: E402

R, D, N, K = 237, 128, 512, 256
LR = 1e-3


def _bce(pos, blocks, labels):
    total = None
    for sc in blocks:
        part = torch.nn.functional.binary_cross_entropy_with_logits(torch.cat([pos.view(-1, 1), sc], 1), labels,
                                                                    reduction="sum") / N
        total = part if total is None else total + part
    return total


def build(arm, E, dev, labels):
    """-> a callable taking (triples, neg_s, neg_o) that performs one training step and returns the loss"""
    torch.manual_seed(0)
    if arm == "torch_sparse":
        ent = torch.nn.Embedding(E, D, sparse=True, device=dev)
        rel = torch.nn.Embedding(R, D, sparse=True, device=dev)
        opt = torch.optim.SparseAdam(list(ent.parameters()) + list(rel.parameters()), lr=LR)

        def step(t, neg_s, neg_o):
            opt.zero_grad(set_to_none=True)
            s, p, o = ent(t[:, 0]), rel(t[:, 1]), ent(t[:, 2])
            pos = (s * p * o).sum(-1)
            sc_s = torch.einsum("nkd,nd->nk", ent(neg_s), p * o)
            sc_o = torch.einsum("nkd,nd->nk", ent(neg_o), s * p)
            loss = _bce(pos, (sc_s, sc_o), labels)
            loss.backward()
            opt.step()
            return loss.detach()
        return step, None
    m = km.create("distmult", E, R, D, device=dev)
    if arm == "sparse_touched":
        opt = kopt.SparseAdam(list(m.parameters()), lr=LR)
        m.set_touched_rows(opt.enable_touched_rows(m.get_s_embedder().weight),
                           opt.enable_touched_rows(m.get_p_embedder().weight))
    else:
        opt = kopt.Adam(list(m.parameters()), lr=LR, device_step=True)

    def loss_fn(t, neg_s, neg_o):
        pos, sc_s, sc_o = m.score_neg_blocks(t[:, 0], t[:, 1], t[:, 2], neg_s, neg_o)
        return _bce(pos, (sc_s, sc_o), labels)
    gs = GraphedStep(loss_fn, opt, warmup=2)
    return gs, gs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--entities", default="14541,4594485")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_adam_probe.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    arms = ("sparse_touched", "adam_dense", "torch_sparse")
    lines = [f"negative-sampling step, DistMult d = {D}, {N} triples per batch, {K} negatives per slot (both slots), bce, "
             f"lr {LR}; ms per step: median (min .. max) of {args.windows} alternated windows of {args.steps} steps, HIP "
             f"events; {torch.cuda.get_device_name(dev)}",
             f"{'entities':>9s}  {'arm':>14s}  {'step':>8s}  {'ms / step':>9s}  {'min':>8s}  {'max':>8s}  last loss"]
    labels = torch.zeros(N, 1 + K, device=dev)
    labels[:, 0] = 1
    for E in (int(x) for x in args.entities.split(",")):
        gc.collect()
        torch.cuda.empty_cache()
        g = torch.Generator().manual_seed(5)
        batches = [(torch.stack([torch.randint(hi, (N,), generator=g) for hi in (E, R, E)], 1).to(dev),
                    torch.randint(E, (N, K), generator=g).to(dev), torch.randint(E, (N, K), generator=g).to(dev))
                   for _ in range(8)]
        steps, graphs = {}, {}
        for arm in arms:
            steps[arm], graphs[arm] = build(arm, E, dev, labels)
            for i in range(8):  # warm-up, capture, first replays
                steps[arm](*batches[i % len(batches)])
        times, last = {arm: [] for arm in arms}, {}
        for _ in range(args.windows):
            for arm in arms:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                for i in range(args.steps):
                    last[arm] = steps[arm](*batches[i % len(batches)])
                t1.record()
                torch.cuda.synchronize()
                times[arm].append(t0.elapsed_time(t1) / args.steps)
        for arm in arms:
            gs = graphs[arm]
            how = "eager" if gs is None else ("captured" if gs.disabled_reason is None and gs.replays > 0 else
                                              f"eager ({gs.disabled_reason})")
            lines.append(f"{E:9d}  {arm:>14s}  {how:>8s}  {statistics.median(times[arm]):9.4f}  {min(times[arm]):8.4f}  "
                         f"{max(times[arm]):8.4f}  {float(last[arm]):.6f}")
            print(lines[-1], flush=True)
        del steps, graphs
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
