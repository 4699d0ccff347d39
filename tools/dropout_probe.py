#!/usr/bin/env python
"""Embedder dropout inside the triple-wise kernels, timed: forward + backward of one slot's negative block
(model.score_neg with a random linear functional) through

  dropout    fused_dropout=True, training mode, dropout 0.2 / 0.1: kge_score_neg_dropout + kge_score_neg_dropout_bwd_accum
  composed   the same model without the option -- the path of the parent commit: n K gathered rows per table, torch
             dropout, score_emb, autograd's scatter-add
  undropped  the same model with dropout 0: kge_score_neg + kge_score_neg_bwd_accum (atomic form: the dropout backward
             has no sorted form), the generator's share is the difference to it

HIP events around `--iters` calls, a warm-up first, `--repeats` windows per route ALTERNATED between the routes (a clock
or thermal drift lands on all three), as tools/score_so_probe.py: the median per-call time in microseconds with min ..
max, one line per case, written to --out (profiles/dropout_probe.txt is one such run).  Shape: FB15k-237's entity count,
d = 128, n = 512, K in {100, 1000}, float32, ComplEx and RotatE, both slots.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from score_so_probe import alternated  # noqa: E402

SHAPES = [(name, 512, 128, K) for name in ("complex", "rotate") for K in (100, 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=237)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dropout_probe: no GPU (a timing needs one)")
    from kge_amd import engine, model
    dev = torch.device("cuda", 0)
    engine.NEG_BWD_SORTED = False
    fmt = lambda t: f"{t[0]:9.1f} us ({t[1]:.1f} .. {t[2]:.1f})"
    lines = ["# dropout_probe: model.score_neg forward + backward of one slot, microseconds per call, median of alternated "
             f"windows (min .. max); E={args.entities}, iters={args.iters}, repeats={args.repeats}, dropout 0.2 / 0.1"]
    for name, n, d, K in SHAPES:
        torch.manual_seed(0)
        mk = lambda fused, pe, pr: model.create(name, args.entities, args.relations, d, device=dev, fused_dropout=fused,
                                                entity_args={"dropout": pe}, relation_args={"dropout": pr}).train()
        models = {"dropout": mk(True, 0.2, 0.1), "composed": mk(False, 0.2, 0.1), "undropped": mk(False, 0.0, 0.0)}
        g = torch.Generator().manual_seed(1)
        s, o = (torch.randint(args.entities, (n,), generator=g).to(dev) for _ in range(2))
        p = torch.randint(args.relations, (n,), generator=g).to(dev)
        neg = torch.randint(args.entities, (n, K), generator=g).to(dev)
        w = torch.randn(n, K, generator=g).to(dev)
        for slot in (0, 2):
            def call(m):
                def fn():
                    m.zero_grad(set_to_none=True)
                    (m.score_neg(s, p, o, slot, neg) * w).sum().backward()
                return fn
            t = alternated({k: call(m) for k, m in models.items()}, args.iters, args.repeats, args.warmup)
            share = t["dropout"][0] - t["undropped"][0]
            lines.append(f"{name:8s} n={n} K={K} d={d} slot={slot}  dropout {fmt(t['dropout'])}  composed {fmt(t['composed'])}  "
                         f"undropped {fmt(t['undropped'])}  generator {share:+.1f} us  composed / dropout "
                         f"x{t['composed'][0] / t['dropout'][0]:.2f}")
            print(lines[-1], flush=True)
        del models
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
