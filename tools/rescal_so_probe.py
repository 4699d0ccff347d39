#!/usr/bin/env python
"""KgeModel.score_so of a RESCAL model (relation prediction) timed through

  composed  RelationalScorer.score_emb(..., "s_o"): repeats to [n R, d] and [n R, d^2] and the spo kernel (the
            reference's generic fallback, kge_model.py:202-209), autograd through the repeats -- the only path of a
            default "rescal" model; reached here with `model.fused_score_so = False`
  fused     create("rescal", ..., grouped=True): kge_score_so / kge_score_so_bwd_accum on the opted-in tables
            (csrc/rescal_so.hip)

at E = 14,541, R = 237, d = 128 and 256: both routes at --n-small pairs (the largest batch at which the composed
repeats fit comfortably: n R d^2 floats, twice with the gradient), and the fused route alone at n = 512 next to the
bytes the composed relation repeat would have needed.  HIP events around `--iters` calls after a warm-up, `--repeats`
windows per route ALTERNATED between the routes: microseconds per call, median (min .. max).  "of f32 MFMA peak" is
2 n R d^2 flops of the forward call over its whole time (launches and the K-split reduction included) against 157.3
TFLOP/s -- an end-to-end rate, not a kernel's.  A shape where the fused route is slower is printed in **bold**.
profiles/rescal_so_probe.txt is one such run."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from score_so_probe import alternated  # noqa: E402  (the alternated-window timer)

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=237)
    ap.add_argument("--n-small", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rescal_so_probe: no GPU (a timing needs one)")
    from kge_amd import model
    dev = torch.device("cuda", 0)
    E, R = args.entities, args.relations
    fmt = lambda t: f"{t[0]:9.1f} us ({t[1]:.1f} .. {t[2]:.1f})"
    lines = ["# rescal_so_probe: microseconds per call, median of alternated windows (min .. max); "
             f"E={E}, R={R}, iters={args.iters}, repeats={args.repeats}"]
    for d in (128, 256):
        torch.manual_seed(0)
        m = model.create("rescal", E, R, d, device=dev, grouped=True).train()
        for n in (args.n_small if d == 128 else max(args.n_small // 4, 1), 512):
            g = torch.Generator().manual_seed(1)
            s, o = (torch.randint(E, (n,), generator=g).to(dev) for _ in range(2))
            w = torch.randn(n, R, generator=g).to(dev)

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

            routes = ("composed", "fused") if n != 512 else ("fused",)
            head = f"rescal n={n} d={d}"
            for grad, what in ((False, "forward           "), (True, "forward + backward")):
                r = alternated({k: call(k == "fused", grad) for k in routes}, args.iters, args.repeats, args.warmup)
                row = f"{head} {what}  fused {fmt(r['fused'])}"
                if "composed" in r:
                    ratio = r["composed"][0] / r["fused"][0]
                    mark = "**" if ratio < 1.0 else ""
                    row += f"  composed {fmt(r['composed'])}  {mark}x{ratio:.2f}{mark}"
                else:
                    row += f"  composed: not run, its relation repeat alone is {n * R * d * d * 4 / 1e9:.2f} GB"
                if not grad:
                    row += f"  [{2.0 * n * R * d * d / (r['fused'][0] * 1e-6) / PEAK_F32_MFMA:.3f} of f32 MFMA peak]"
                lines.append(row)
                print(row, flush=True)
            m.fused_score_so = True
        del m
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
