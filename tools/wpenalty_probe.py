#!/usr/bin/env python3
"""What folding the frequency-weighted penalty terms into the optimizer's pass does to the
negative-sampling training step: DistMult, n = 512 triples per batch, K = 256 uniform negatives per slot, both slots,
d = 128, bce loss on every slot's [n, 1 + K] block, Adagrad, a weighted L3 term on the entity and on the relation
table (lookup_embedder.regularize_args.weighted), for an entity table of 14,541 rows (the FB15k-237 shape) and of
4,594,485 rows.  Per table size four arms that take the same steps:
  eager_autograd   the path without the feature: the term as lookup_embedder.py:148-173 computes it (torch.unique with
                   counts, the gather, ** p * counts, / len(indexes)) back-propagated with the loss, a dense Adagrad
                   step, everything issued from Python (such a job cannot be captured: unique waits for the host)
  folded_eager     kge_penalty_count + kge_adagrad_step_multi_wpenalty, issued from Python
  folded_captured  the same step captured once and replayed (kge_amd.train_graph.GraphedStep)
  folded_touched   captured, the entity table on the touched-row step (kge_adagrad_step_touched_wpenalty)
ms per step: median and min..max of `--windows` windows of `--steps` steps; the windows of the four arms ALTERNATE (arm
1 window 1, arm 2 window 1, ..., arm 1 window 2, ...), HIP events around each window.  The traced penalty value of the
last step is printed per arm as a check.

Then the count kernel alone, kge_penalty_count with the in-wave duplicate merge (the default) and with one atomic per
lane (switch PENALTY_COUNT_PLAIN), on three inputs of `--count-n` ids over 14,541 rows: one id repeated, uniform random
ids, and ids drawn from 16 rows; us per launch, median (min .. max) of alternated windows of 200 launches.

    python tools/wpenalty_probe.py [--windows 7] [--steps 30] [--entities 14541,4594485] [--out FILE]
Writes its table to profiles/wpenalty_probe.txt (or --out)."""
import argparse
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kge_amd import _lib, engine, model as km, optim as kopt  # noqa: E402
from kge_amd.train_graph import GraphedStep  # noqa: E402

R, D, N, K = 237, 128, 512, 256
P_NORM, W_ENT, W_REL = 3, 1e-2, 5e-2
ARMS = ("eager_autograd", "folded_eager", "folded_captured", "folded_touched")


def _reference_term(weight, indexes, regularize_weight):
    """lookup_embedder.py:148-173, lp with an odd p."""
    unique_indexes, counts = torch.unique(indexes, return_counts=True)
    parameters = torch.abs(weight[unique_indexes])
    return (regularize_weight / P_NORM * (parameters ** P_NORM * counts.float().view(-1, 1))).sum() / len(indexes)


class Arm:
    def __init__(self, name, E, dev):
        torch.manual_seed(0)
        self.name = name
        self.m = m = km.create("distmult", E, R, D, device=dev)
        self.ent, self.rel = m.get_s_embedder().weight, m.get_p_embedder().weight
        self.opt = opt = kopt.Adagrad(list(m.parameters()), lr=0.1)
        folded = name != "eager_autograd"
        if name == "folded_touched":
            m.set_touched_rows(opt.enable_touched_rows(self.ent))
        if folded:
            opt.set_penalty(self.ent, "lp", P_NORM, W_ENT, weighted=True)
            opt.set_penalty(self.rel, "lp", P_NORM, W_REL, weighted=True)
        labels = torch.zeros(N, 1 + K, device=dev)
        labels[:, 0] = 1
        self.last_pen = None

        def loss_fn(t, neg_s, neg_o):
            if folded:  # the counts (and, on the touched-row step, the row marks) the step reads
                opt.count_penalty(self.rel, t[:, 1], N)
                opt.count_penalty(self.ent, t[:, 0], N)
                opt.count_penalty(self.ent, t[:, 2], N)
            pos, sc_s, sc_o = m.score_neg_blocks(t[:, 0], t[:, 1], t[:, 2], neg_s, neg_o)
            total = None
            for sc in (sc_s, sc_o):
                part = torch.nn.functional.binary_cross_entropy_with_logits(
                    torch.cat([pos.view(-1, 1), sc], 1), labels, reduction="sum") / N
                total = part if total is None else total + part
            if not folded:
                pen = (_reference_term(self.rel, t[:, 1], W_REL)
                       + _reference_term(self.ent, torch.cat((t[:, 0].view(-1, 1), t[:, 2].view(-1, 1)), 1), W_ENT))
                self.last_pen = pen.detach()
                total = total + pen
            return total
        g = torch.Generator().manual_seed(5)
        self.batches = [(torch.stack([torch.randint(hi, (N,), generator=g) for hi in (E, R, E)], 1).to(dev),
                         torch.randint(E, (N, K), generator=g).to(dev), torch.randint(E, (N, K), generator=g).to(dev))
                        for _ in range(8)]
        self.step = GraphedStep(loss_fn, opt, warmup=2, enabled=name in ("folded_captured", "folded_touched"))
        for i in range(8):  # warm-up, capture, first replays
            self.step(*self.batches[i % 8])
        self.times = []

    def window(self, steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for i in range(steps):
            self.step(*self.batches[i % 8])
        t1.record()
        torch.cuda.synchronize()
        self.times.append(t0.elapsed_time(t1) / steps)

    def penalty(self):
        if self.name == "eager_autograd":
            return float(self.last_pen)
        return float(self.opt.penalty_value(self.ent)) + float(self.opt.penalty_value(self.rel))


def count_probe(args, dev, lines):
    V, n = 14541, args.count_n
    g = torch.Generator().manual_seed(9)
    inputs = {"one id repeated": torch.full((n,), 4711, dtype=torch.int64),
              "uniform random": torch.randint(V, (n,), generator=g),
              "16 distinct rows": torch.randint(16, (n,), generator=g) * 907}
    counts = engine.penalty_counts(V, dev)
    lines.append("")
    lines.append(f"kge_penalty_count alone, {n} int64 ids over {V} rows, us per launch: median (min .. max) of "
                 f"{args.windows} alternated windows of 200 launches")
    lines.append(f"{'input':>18s}  {'merge us':>9s}  {'min':>7s}  {'max':>7s}  {'plain us':>9s}  {'min':>7s}  {'max':>7s}")
    for name, ids in inputs.items():
        ids = ids.to(dev)
        times = {0: [], 1: []}
        for w in range(args.windows + 1):
            for plain in (0, 1):
                with _lib.switches(PENALTY_COUNT_PLAIN=plain):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0.record()
                    for _ in range(200):
                        engine.penalty_count(ids, counts, V)
                    t1.record()
                    torch.cuda.synchronize()
                if w > 0:  # (the first window of each form warms up)
                    times[plain].append(t0.elapsed_time(t1) * 1000.0 / 200)
        counts.zero_()
        a, b = times[0], times[1]
        lines.append(f"{name:>18s}  {statistics.median(a):9.2f}  {min(a):7.2f}  {max(a):7.2f}  "
                     f"{statistics.median(b):9.2f}  {min(b):7.2f}  {max(b):7.2f}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--count-n", type=int, default=1024)
    ap.add_argument("--entities", default="14541,4594485")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpenalty_probe.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"negative-sampling step with weighted L{P_NORM} terms on both tables, DistMult d = {D}, {N} triples per "
             f"batch, {K} negatives per slot (both slots), bce, Adagrad; ms per step: median (min .. max) of "
             f"{args.windows} alternated windows of {args.steps} steps, HIP events; {torch.cuda.get_device_name(dev)}",
             f"{'entities':>9s}  {'arm':>16s}  {'ms / step':>9s}  {'min':>8s}  {'max':>8s}  {'replays':>7s}  last penalty"]
    for E in (int(x) for x in args.entities.split(",")):
        gc.collect()
        torch.cuda.empty_cache()
        arms = [Arm(name, E, dev) for name in ARMS]
        for _ in range(args.windows):
            for arm in arms:
                arm.window(args.steps)
        for arm in arms:
            why = arm.step.disabled_reason
            lines.append(f"{E:9d}  {arm.name:>16s}  {statistics.median(arm.times):9.4f}  {min(arm.times):8.4f}  "
                         f"{max(arm.times):8.4f}  {arm.step.replays:7d}  {arm.penalty():.6f}"
                         + (f"  ({why})" if why else ""))
            print(lines[-1], flush=True)
        del arms
    count_probe(args, dev, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
