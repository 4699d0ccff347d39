#!/usr/bin/env python
"""KgeModel.score_so (relation prediction, kge_model.py:727-747) timed through

  composed  the path of the parent commit: RelationalScorer.score_emb(..., "s_o") -- repeat_interleave / repeat to three
            [n R, d] tensors and the spo kernel (the reference's generic fallback, kge_model.py:202-209), autograd
            through the repeats; reached here with `model.fused_score_so = False`
  fused     kge_score_so (+ kge_score_so_bwd_accum): engine.score_so on the tables, model.score_so without a gradient,
            model.score_so with backward

HIP events around `--iters` calls, a warm-up first, `--repeats` windows per route ALTERNATED between the two routes (a
clock or thermal drift lands on both): the median per-call time in microseconds and the spread are printed, one line
per case, with torch.cuda.max_memory_allocated of one forward + backward of each route, and written to --out
(profiles/score_so_probe.txt is one such run).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = [("complex", 1.0, 512, 128, 237), ("transe", 1.0, 512, 128, 237), ("rotate", 1.0, 512, 128, 237),
          ("complex", 1.0, 512, 128, 474), ("transe", 1.0, 512, 128, 474), ("rotate", 1.0, 512, 128, 474),
          ("complex", 1.0, 512, 128, 822), ("transe", 1.0, 512, 128, 822), ("rotate", 1.0, 512, 128, 822),
          ("complex", 1.0, 100, 128, 237)]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # microseconds per call


def alternated(fns, iters, repeats, warmup):
    """{route: (median, min, max)} of `repeats` windows per route, the routes taking turns"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in out.items()}


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_so_probe: no GPU (a timing needs one)")
    from kge_amd import engine, model
    dev = torch.device("cuda", 0)
    fmt = lambda t: f"{t[0]:9.1f} us ({t[1]:.1f} .. {t[2]:.1f})"
    lines = ["# score_so_probe: microseconds per call, median of alternated windows (min .. max); "
             f"E={args.entities}, iters={args.iters}, repeats={args.repeats}"]
    for name, lp, n, d, R in SHAPES:
        torch.manual_seed(0)
        m = model.create(name, args.entities, R, d, l_norm=lp, device=dev).train()
        g = torch.Generator().manual_seed(1)
        s, o = (torch.randint(args.entities, (n,), generator=g).to(dev) for _ in range(2))
        w = torch.randn(n, R, generator=g).to(dev)
        t = m.tables()

        def call(fused, grad):
            def fn():
                m.fused_score_so = fused
                if grad:
                    m.zero_grad(set_to_none=True)
                    (m.score_so(s, o) * w).sum().backward()
                else:
                    with torch.no_grad():
                        m.score_so(s, o)
            return fn

        eng = alternated({"engine": lambda: engine.score_so(t, s, o)}, args.iters, args.repeats, args.warmup)["engine"]
        fwd = alternated({"composed": call(False, False), "fused": call(True, False)}, args.iters, args.repeats, args.warmup)
        fb = alternated({"composed": call(False, True), "fused": call(True, True)}, args.iters, args.repeats, args.warmup)
        mem = {k: peak(call(k == "fused", True)) for k in ("composed", "fused")}
        m.fused_score_so = True
        head = f"{name:8s} n={n} d={d} R={R}"
        lines += [f"{head} engine.score_so            {fmt(eng)}",
                  f"{head} model.score_so no grad     composed {fmt(fwd['composed'])}  fused {fmt(fwd['fused'])}  "
                  f"x{fwd['composed'][0] / fwd['fused'][0]:.2f}",
                  f"{head} model.score_so + backward  composed {fmt(fb['composed'])}  fused {fmt(fb['fused'])}  "
                  f"x{fb['composed'][0] / fb['fused'][0]:.2f}",
                  f"{head} peak memory of fwd + bwd   composed {mem['composed'] / 1e6:8.1f} MB  fused {mem['fused'] / 1e6:8.1f} MB"]
        print("\n".join(lines[-4:]), flush=True)
        del m
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
