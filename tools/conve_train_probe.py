#!/usr/bin/env python
"""Time and peak memory of ConvE's training path at the FB15k-237 shape (E = 14,541, d = 200: h = 10, w = 20, fs = 3,
pad = 0, feature-map dropout 0.2, projection dropout 0.3) at n = 128 and n = 512, float32: forward + backward of

  (a) the network alone (ConveNetOps.network on gathered rows, the gradient of sum(x^2)), and
  (b) a whole score_sp step (model.ConvE.score_sp, the gradient of sum(scores^2) into every parameter),

on the fused route (fused_train=True: kge_conve_train_fwd / kge_conve_train_bwd) against the torch route (the same model
class without the option) on the same GPU.  HIP events around `--iters` steps after a warm-up step; the two routes take
their windows in turn, `--repeats` windows each; median (min .. max) in microseconds per step.  Peak memory:
torch.cuda.max_memory_allocated over one score_sp step, above what was allocated before it.  Writes
profiles/conve_train_probe.txt."""
import argparse
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from conve_probe import DEV, fmt, timed_in_turn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=474)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--ns", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conve_train_probe.txt"))
    args = ap.parse_args()
    from kge_amd import model
    E, R, d = args.entities, args.relations, args.dim
    torch.manual_seed(0)
    ms = [model.create("conve", E, R, d, device=DEV, fused_train=ft).train() for ft in (True, False)]
    ms[1].load_state_dict(ms[0].state_dict())
    sc = ms[0].get_scorer()
    lines = [f"conve_train_probe: E={E} R={R} d={d} (h={sc.emb_height}, w={sc.emb_width}, fs={sc.filter_size}, "
             f"pad={sc.padding}, F={sc.projection.weight.shape[1]}) float32, forward + backward, us per step: median "
             f"(min .. max) of {args.repeats} windows of {args.iters} steps; {torch.cuda.get_device_name(0)}"]
    for n in args.ns:
        g = torch.Generator().manual_seed(n)
        s, p = (torch.randint(0, hi, (n,), generator=g).to(DEV) for hi in (E, R))

        def net_step(m):
            rows = [m.get_s_embedder().weight[s].detach().requires_grad_(), m.get_p_embedder().weight[p].detach().requires_grad_()]
            m.get_scorer().network(*rows).square().sum().backward()

        def sp_step(m):
            m.zero_grad(set_to_none=True)
            m.score_sp(s, p).square().sum().backward()

        def peak(m):
            sp_step(m)
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            sp_step(m)
            torch.cuda.synchronize()
            return (torch.cuda.max_memory_allocated() - base) / 1e6

        t_net = timed_in_turn([lambda: net_step(ms[0]), lambda: net_step(ms[1])], args.iters, args.repeats)
        t_sp = timed_in_turn([lambda: sp_step(ms[0]), lambda: sp_step(ms[1])], args.iters, args.repeats)
        assert ms[0].routes["train"] > 0 and ms[1].routes.get("train") is None
        lines.append(f"n={n}:")
        for what, t in (("network alone", t_net), ("score_sp step", t_sp)):
            lines.append(f"  {what}   fused {fmt(t[0])}   torch {fmt(t[1])}   torch / fused {t[1][0] / t[0][0]:.2f}")
        lines.append(f"  peak memory of a score_sp step above the model: fused {peak(ms[0]):.1f} MB   torch {peak(ms[1]):.1f} MB")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
