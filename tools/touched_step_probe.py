#!/usr/bin/env python3
"""What stepping only the touched entity rows (kge_amd.optim.Adagrad.enable_touched_rows) does to
the negative-sampling training step: DistMult, n = 512 triples per batch, K = 256 uniform negatives per slot, both
slots, d = 128, bce loss on every slot's [n, 1 + K] block, Adagrad -- the whole step captured once and replayed
(kge_amd.train_graph.GraphedStep), for an entity table of 14,541 rows (the FB15k-237 shape) and of 4,594,485 rows
(SURVEY's C5 shape).  Per table size two arms that take the same steps:
  off   the dense path: every backward node fills a zeros_like(ent), kge_adagrad_step_multi sweeps both tables
  on    the entity gradient in the persistent buffer, rows marked (kge_touched_mark), kge_adagrad_step_touched
ms per replayed step: median and min..max of `--windows` windows of `--steps` replays, HIP events around each window.
The loss of the last step of both arms is printed as a check (the arms differ in the order of float atomics only).

    python tools/touched_step_probe.py [--windows 9] [--steps 40] [--entities 14541,4594485] [--out FILE]
Writes its table to profiles/touched_step_probe.txt (or --out)."""
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


def run(E, touched, args, dev):
    torch.manual_seed(0)
    m = km.create("distmult", E, R, D, device=dev)
    ent = m.get_s_embedder().weight
    opt = kopt.Adagrad(list(m.parameters()), lr=0.1)
    if touched:
        m.set_touched_rows(opt.enable_touched_rows(ent))
    labels = torch.zeros(N, 1 + K, device=dev)
    labels[:, 0] = 1

    def loss_fn(t, neg_s, neg_o):
        pos, sc_s, sc_o = m.score_neg_blocks(t[:, 0], t[:, 1], t[:, 2], neg_s, neg_o)
        total = None
        for sc in (sc_s, sc_o):
            part = torch.nn.functional.binary_cross_entropy_with_logits(torch.cat([pos.view(-1, 1), sc], 1), labels,
                                                                        reduction="sum") / N
            total = part if total is None else total + part
        return total
    g = torch.Generator().manual_seed(5)
    batches = [(torch.stack([torch.randint(hi, (N,), generator=g) for hi in (E, R, E)], 1).to(dev),
                torch.randint(E, (N, K), generator=g).to(dev), torch.randint(E, (N, K), generator=g).to(dev))
               for _ in range(8)]
    step = GraphedStep(loss_fn, opt, warmup=2)
    for i in range(8):  # warm-up, capture, first replays
        step(*batches[i % len(batches)])
    times = []
    for _ in range(args.windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for i in range(args.steps):
            loss = step(*batches[i % len(batches)])
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / args.steps)
    peak = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    if touched:
        grad, bitmap = opt.touched_rows(ent)
        assert ent.grad is None and not bitmap.any() and not grad.view(-1)[::4099].any(), "buffer or bitmap not zero"
    return times, float(loss), step.replays, step.disabled_reason, peak  # (not the step: it holds the tables)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--entities", default="14541,4594485")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "touched_step_probe.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"negative-sampling step, DistMult d = {D}, {N} triples per batch, {K} negatives per slot (both slots), bce, "
             f"Adagrad; captured step, ms per replay: median (min .. max) of {args.windows} windows of {args.steps} "
             f"replays, HIP events; {torch.cuda.get_device_name(dev)}",
             f"{'entities':>9s}  {'touched_rows':>12s}  {'ms / step':>9s}  {'min':>8s}  {'max':>8s}  {'replays':>7s}  "
             f"{'peak GiB':>8s}  last loss"]
    for E in (int(x) for x in args.entities.split(",")):
        for touched in (False, True):
            gc.collect()  # the previous arm's tables, gradient buffers and graph are gone before this one allocates
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            times, loss, replays, why, peak = run(E, touched, args, dev)
            lines.append(f"{E:9d}  {'on' if touched else 'off':>12s}  {statistics.median(times):9.4f}  {min(times):8.4f}  "
                         f"{max(times):8.4f}  {replays:7d}  {peak:8.2f}  {loss:.6f}" + (f"  ({why})" if why else ""))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
