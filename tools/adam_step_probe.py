#!/usr/bin/env python3
"""What kge_amd.optim.Adam(device_step=True) buys on the 1vsAll training step at the FB15k-237 shape (14,541 x 237,
d = 256, 512 triples per batch; bf16 scoring, fused cross entropy of both directions): seconds per 100 batches, timed
with HIP events over several windows, for
  host    eager steps with the host-step Adam (bias correction on the host, one launch per table: the only form before)
  device  eager steps with device_step=True (clock kernel + ONE update launch over both tables)
  graph   device_step=True under GraphedStep: the whole step as one hipGraph replay
The three arms take the same steps; the loss after the last batch is printed as a check.

    python tools/adam_step_probe.py [--windows 5] [--batches 100] [--penalty]
--penalty: lp (p = 2) terms on both tables -- back-propagated through autograd in the host arm (what a job has to do
there), folded into the optimizer's launch in the other two."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kge_amd import model as km, optim as kopt  # noqa: E402
from kge_amd.train_graph import GraphedStep  # noqa: E402

E, R, D, N = 14541, 237, 256, 512
WEIGHT = 1e-4


def run(arm, args, batches, dev):
    torch.manual_seed(0)
    m = km.create("complex", E, R, D, device=dev, score_dtype=torch.bfloat16)
    params = list(m.parameters())
    opt = kopt.Adam(params, lr=0.003, bf16_copies=True, device_step=arm != "host")
    if args.penalty and arm != "host":
        for p in params:
            opt.set_penalty(p, "lp", 2, WEIGHT)

    def loss_fn(t):
        loss = m.loss_sp_po_sum(t[:, 0], t[:, 1], t[:, 2], 1.0 / N)
        if args.penalty and arm == "host":
            loss = loss + sum(WEIGHT / 2 * (p * p).sum() for p in params)
        return loss
    step = GraphedStep(loss_fn, opt, warmup=2, enabled=arm == "graph")
    for b in batches[:10]:  # warm-up, capture
        step(b)
    times = []
    for _ in range(args.windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for b in batches:
            loss = step(b)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / 1e3)
    return times, float(loss), step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--penalty", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    batches = [torch.stack([torch.randint(hi, (N,), generator=g) for hi in (E, R, E)], 1).to(dev)
               for _ in range(args.batches)]
    print(f"1vsAll step, ComplEx {E} x {R}, d = {D}, {N} triples per batch, Adam lr 0.003"
          f"{', lp penalties on both tables' if args.penalty else ''}; seconds per {args.batches} batches, "
          f"{args.windows} windows")
    for arm in ("host", "device", "graph"):
        times, loss, step = run(arm, args, batches, dev)
        print(f"{arm:7s} median {statistics.median(times):.4f}  min {min(times):.4f}  max {max(times):.4f}  "
              f"last loss {loss:.6f}  replays {step.replays}" + (f"  ({step.disabled_reason})" if step.disabled_reason else ""))


if __name__ == "__main__":
    main()
