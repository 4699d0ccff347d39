#!/usr/bin/env python
"""Time of a filtered top-k prediction batch, the fused entry against the route it replaces, on the same tables:

  fused      engine.topk (kge_topk: scoring, filter and per-row top-k in one kernel + the merge; no score matrix)
  composed   engine.score_sp (the [n, E] float32 matrix), the known answers masked to -inf with one index_put, torch.topk

at the FB15k-237 shape (14,541 entities) and one large-table shape (default 1,000,000 entities), ComplEx at d = 128 on
float32 tables (the exact chain on both routes), n = 512 queries, k = 10 and k = 128, one filter set with ~8 known
answers per row.  HIP events around `--iters` calls, median (min .. max) of `--repeats` windows, in ms per call.
Writes profiles/topk_probe.txt.  Note the composed route's order among equal scores is torch.topk's (unspecified); the
probe compares ids only on rows without ties at the cut.

--wide: the two kernel pairs of kge_topk against each other and against the composed route, k in 10 .. 1024 (the narrow
pair of topk.hip forced by switch TOPK_WIDE = 2 where k <= 128, the wide pair of topk_wide.hip by TOPK_WIDE = 1), the
windows of the three routes ALTERNATED, plus the workspace bytes of each pair.  Writes profiles/topk_wide_probe.txt."""
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


def timed_alternated(fns, iters, repeats):
    """[(median, min, max)] per function: one window of each in turn, `repeats` rounds."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for o, fn in zip(out, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            o.append(a.elapsed_time(b) / iters)
    return [(float(np.median(o)), min(o), max(o)) for o in out]


def wide_rows(engine, T, E, n, s, p, filt, rows, col, iters, repeats):
    """The --wide lines of one table size."""
    import ctypes
    from kge_amd import _lib
    lines = []
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f} .. {t[2]:.4f})"
    for k in (10, 32, 64, 128, 256, 1024):
        def fused(which):
            def run():
                with _lib.switches(TOPK_WIDE=which):
                    return engine.topk(T, "sp_", s, p, k, [filt])
            return run

        def composed():
            sc = engine.score_sp(T, s, p)
            sc.index_put_((rows, col), torch.tensor(float("-inf"), device=DEV))
            return torch.topk(sc, k, dim=1)
        names = (["narrow"] if k <= 128 else []) + ["wide", "composed"]
        fns = ([fused(2)] if k <= 128 else []) + [fused(1), composed]
        wv, wi = fns[-2]()
        cv, ci = composed()
        cut_tie = (cv[:, -1:] == cv).sum(dim=1) > 1
        # (torch.topk leaves the order among equal scores open: values bit for bit, ids as sets off the cut)
        agree = bool(torch.equal(wv.view(torch.int32), cv.view(torch.int32))) and \
            bool(((wi.sort(dim=1).values == ci.sort(dim=1).values).all(dim=1) | cut_tie).all())
        pairs = "-"
        if k <= 128:
            nv, ni = fns[0]()
            pairs = bool(torch.equal(ni, wi)) and bool(torch.equal(nv.view(torch.int32), wv.view(torch.int32)))
        ws = {}
        tc = T.c(0)
        for name, which in (("narrow", 2), ("wide", 1)):
            if name in names:
                with _lib.switches(TOPK_WIDE=which):
                    ws[name] = _lib.lib().kge_topk_workspace_bytes(ctypes.byref(tc), n, E, k, 1)
        times = timed_alternated(fns, iters, repeats)
        lines.append(f"E={E:>9,} k={k:>4}  " + "   ".join(f"{nm} {fmt(t)}" for nm, t in zip(names, times)) +
                     "   workspace " + " / ".join(f"{nm} {b / 2 ** 20:,.1f} MiB" for nm, b in ws.items()) +
                     f"   score matrix {n * E * 4 / 2 ** 20:,.0f} MiB   wide = composed: {agree}   narrow = wide bit for bit: {pairs}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, nargs="*", default=[14541, 1000000])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--wide", action="store_true", help="narrow pair / wide pair / composed, k = 10 .. 1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "topk_wide_probe.txt" if args.wide else "topk_probe.txt")
    from kge_amd import engine
    lines = [f"topk_probe: complex d={args.dim} float32, n={args.n}, one filter set (8 per row), ms per call: "
             f"median (min .. max) of {args.repeats} windows of {args.iters} calls" + (", windows alternated" if args.wide else "")]
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
        if args.wide:
            lines += wide_rows(engine, T, E, n, s, p, (begin, end, col), rows, col, args.iters, args.repeats)
        for k in () if args.wide else (10, 128):
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
