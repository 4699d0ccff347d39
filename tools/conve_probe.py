#!/usr/bin/env python
"""Time of ConvE's evaluation path at the FB15k-237 shape (E = 14,541, d = 200: h = 10, w = 20, fs = 3, pad = 0) at
n = 512 and n = 100, float32:

  (a) kge_conve_queries alone (engine.conve_queries) against the torch eval-mode operation sequence of the network
      (cat, conv2d, batch_norm, relu, linear, batch_norm, relu) on the same GPU;
  (b) the whole score_sp on the kernel route (model.ConvE under no_grad) against the torch sequence with mm + bias, and
      against float32 DistMult score_sp at the same width (d = 200).

HIP events around `--iters` calls (default 1000: windows of 0.1 - 0.2 s) after a warm-up call; the variants that are
compared take their windows in turn (kernel, torch, kernel, torch, ...), `--repeats` windows each; median (min .. max)
in microseconds per call, so the spread stands next to every ratio.  Writes profiles/conve_probe.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"


def timed_in_turn(fns, iters, repeats):
    """the windows of several variants alternated: [median, min, max] per variant"""
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
    return [(float(np.median(o)), min(o), max(o)) for o in out]


def fmt(t):
    return f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=474)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--ns", type=int, nargs="+", default=[512, 100])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conve_probe.txt"))
    args = ap.parse_args()
    from kge_amd import engine, model
    E, R, d = args.entities, args.relations, args.dim
    torch.manual_seed(0)
    m = model.create("conve", E, R, d, device=DEV).eval()
    sc = m.get_scorer()
    with torch.no_grad():
        sc.bn1.running_var.uniform_(0.5, 1.5)
        sc.bn2.running_var.uniform_(0.5, 1.5)
    dm = model.create("distmult", E, R, d, device=DEV).eval()
    ent, rel = m.get_s_embedder().weight.detach(), m.get_p_embedder().weight.detach()
    F = sc.projection.weight.shape[1]
    lines = [f"conve_probe: E={E} R={R} d={d} (h={sc.emb_height}, w={sc.emb_width}, fs={sc.filter_size}, "
             f"pad={sc.padding}, F={F}) float32, us per call: median (min .. max) of {args.repeats} windows of "
             f"{args.iters} calls; {torch.cuda.get_device_name(0)}"]
    with torch.no_grad():
        for n in args.ns:
            g = torch.Generator().manual_seed(n)
            s, p = (torch.randint(0, hi, (n,), generator=g).to(DEV) for hi in (E, R))
            net = sc.kernel_net()

            def torch_sp():
                return torch.mm(sc.network(ent[s], rel[p]), ent[:, 1:].t()) + ent[:, 0]
            assert m.kernel_route()
            t_q, t_net = timed_in_turn([lambda: engine.conve_queries(net, ent, rel, s, p),
                                        lambda: sc.network(ent[s], rel[p])], args.iters, args.repeats)
            t_sp, t_ref, t_dm = timed_in_turn([lambda: m.score_sp(s, p), torch_sp, lambda: dm.score_sp(s, p)],
                                              args.iters, args.repeats)
            err = float((m.score_sp(s, p) - torch_sp()).abs().max())
            lines.append(f"n={n}: projection 2 n F d = {2 * n * F * d / 1e9:.2f} GF; channel partials "
                         f"{32 * n * d * 4 / 1e6:.1f} MB")
            lines.append(f"  query network   kge_conve_queries {fmt(t_q)}   torch eval-mode ops {fmt(t_net)}   "
                         f"torch / kernel {t_net[0] / t_q[0]:.2f}")
            lines.append(f"  score_sp        kernel route      {fmt(t_sp)}   torch ops + mm      {fmt(t_ref)}   "
                         f"torch / kernel {t_ref[0] / t_sp[0]:.2f}   max |difference| {err:.2e}")
            lines.append(f"                  float32 DistMult score_sp, d = {d}: {fmt(t_dm)}   ConvE / DistMult "
                         f"{t_sp[0] / t_dm[0]:.2f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
