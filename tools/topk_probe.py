#!/usr/bin/env python
"""Time of a filtered top-k prediction batch, the fused entry against the route it replaces, on the same tables:

  fused      engine.topk (kge_topk: scoring, filter and per-row top-k in one kernel + the merge; no score matrix)
  composed   engine.score_sp (the [n, E] float32 matrix), the known answers masked to -inf with one index_put, torch.topk

at the FB15k-237 shape (14,541 entities) and one large-table shape (default 1,000,000 entities), ComplEx at d = 128 on
float32 tables (the exact chain on both routes), n = 512 queries, k = 10 and k = 128, one filter set with ~8 known
answers per row.  HIP events around `--iters` calls, median (min .. max) of `--repeats` windows, in ms per call.
Writes profiles/topk_probe.txt.  Note the composed route's order among equal scores is torch.topk's (unspecified); the
probe compares ids only on rows without ties at the cut."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"


def timed(fn, iters, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, nargs="*", default=[14541, 1000000])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_probe.txt"))
    args = ap.parse_args()
    from kge_amd import engine
    lines = [f"topk_probe: complex d={args.dim} float32, n={args.n}, one filter set (8 per row), ms per call: "
             f"median (min .. max) of {args.repeats} windows of {args.iters} calls"]
    for E in args.entities:
        g = torch.Generator().manual_seed(0)
        ent = (torch.randn(E, args.dim, generator=g) * 0.3).to(DEV)
        rel = (torch.randn(237, args.dim, generator=g) * 0.3).to(DEV)
        T = engine.Tables("complex", ent, rel)
        n = args.n
        s = torch.randint(0, E, (n,), generator=g).to(DEV)
        p = torch.randint(0, 237, (n,), generator=g).to(DEV)
        begin = (torch.arange(n) * 8).to(DEV)
        end = begin + 8
        col = torch.randint(0, E, (n * 8,), generator=g).to(DEV)
        rows = torch.arange(n, device=DEV).repeat_interleave(8)
        for k in (10, 128):
            def fused():
                return engine.topk(T, "sp_", s, p, k, [(begin, end, col)])

            def composed():
                sc = engine.score_sp(T, s, p)
                sc.index_put_((rows, col), torch.tensor(float("-inf"), device=DEV))
                return torch.topk(sc, k, dim=1)
            fv, fi = fused()
            cv, ci = composed()
            cut_tie = (cv[:, -1:] == cv).sum(dim=1) > 1
            agree = bool(((fi == ci).all(dim=1) | cut_tie).all())
            tf, tc = timed(fused, args.iters, args.repeats), timed(composed, args.iters, args.repeats)
            lines.append(f"E={E:>9,} k={k:>3}  fused {tf[0]:.4f} ({tf[1]:.4f} .. {tf[2]:.4f})   composed {tc[0]:.4f} "
                         f"({tc[1]:.4f} .. {tc[2]:.4f})   score matrix {n * E * 4 / 2 ** 20:,.0f} MiB   ids agree: {agree}")
        del T, ent, rel
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
