#!/usr/bin/env python
"""Time of the relation-grouped RESCAL entries beside the ungrouped ones at E = 14,541, n = 512, K = 256, d = 128 and
256, with the batch's relation ids drawn for R = 237 (FB15k-237: small groups) and for R = 11 (WN18RR: groups of dozens):

  kge_rescal_queries        against kge_rescal_queries_grouped (grouping included);
  kge_score_neg_bwd_accum   against kge_score_neg_bwd_accum_grouped (grouping and the grouped build included);
  DistMult's kge_score_neg_bwd_accum on the same entity table beside both.

The candidates of a row are timed in ALTERNATED windows (a, b, c, a, b, c, ...) of `--iters` calls between HIP events
after a warm-up call each, so that clock and cache state drift hits them alike; median (min .. max) of `--repeats`
windows, microseconds per call.  Writes profiles/rescal_grouped_probe.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"


def alternated(fns, iters, repeats):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(1e3 * a.elapsed_time(b) / iters)
    return [(float(np.median(x)), min(x), max(x)) for x in out]


def fmt(t):
    return f"{t[0]:8.1f} ({t[1]:.1f} .. {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, nargs="+", default=[237, 11])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--negatives", type=int, default=256)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescal_grouped_probe.txt"))
    args = ap.parse_args()
    from kge_amd import engine
    E, n, K = args.entities, args.n, args.negatives
    lines = [f"rescal_grouped_probe: E={E} n={n} K={K} float32, us per call: median (min .. max) of {args.repeats} "
             f"alternated windows of {args.iters} calls; {torch.cuda.get_device_name(0)}"]
    for d in args.dims:
        for R in args.relations:
            g = torch.Generator().manual_seed(0)
            ent = (torch.randn(E, d, generator=g) * 0.3).to(DEV)
            rel = (torch.randn(R, d * d, generator=g) * 0.1).to(DEV)
            rel_d = (torch.randn(R, d, generator=g) * 0.3).to(DEV)
            s, p, o = (torch.randint(0, hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
            neg = torch.randint(0, E, (n, K), generator=g).to(DEV)
            gneg = torch.randn(n, K, generator=g).to(DEV)
            tr, td = engine.Tables("rescal", ent, rel), engine.Tables("distmult", ent, rel_d)
            groups = int(torch.unique(p).numel())
            lines.append(f"d={d} R={R}: {groups} groups, {n / groups:.1f} rows per group")
            for direction, a in (("sp_", s), ("_po", o)):
                plain, grouped = alternated([lambda: engine.rescal_queries(tr, direction, a, p),
                                             lambda: engine.rescal_queries(tr, direction, a, p, grouped=True)],
                                            args.iters, args.repeats)
                lines.append(f"  queries {direction}      ungrouped {fmt(plain)}   grouped {fmt(grouped)}   "
                             f"grouped / ungrouped {grouped[0] / plain[0]:.2f}")
            for slot in (2, 0):
                ge, gr = torch.zeros_like(ent), torch.zeros_like(rel)
                ged, grd = torch.zeros_like(ent), torch.zeros_like(rel_d)
                plain, grouped, dist = alternated(
                    [lambda: engine.score_neg_bwd_accum(tr, s, p, o, slot, neg, gneg, None, ge, gr),
                     lambda: engine.score_neg_bwd_accum_grouped(tr, s, p, o, slot, neg, gneg, None, ge, gr),
                     lambda: engine.score_neg_bwd_accum(td, s, p, o, slot, neg, gneg, None, ged, grd)],
                    args.iters, args.repeats)
                lines.append(f"  neg_bwd slot {slot}    ungrouped {fmt(plain)}   grouped {fmt(grouped)}   "
                             f"grouped / ungrouped {grouped[0] / plain[0]:.2f}   distmult {fmt(dist)}   "
                             f"ungrouped / distmult {plain[0] / dist[0]:.2f}   grouped / distmult {grouped[0] / dist[0]:.2f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
