#!/usr/bin/env python
"""Time of the Relational Tucker3 paths at the FB15k-237 shape (E = 14,541, R = 237, n = 512, d_r = 100) at d = 128 and
d = 256:

  kge_tucker3_project, all R rows and the batch's gathered rows, beside the bytes it writes over 8 TB/s;
  score_sp, score_sp_po, score_neg (K = 256) and the backward of each through model.RelationalTucker3 on both routes,
  beside (a) model.Rescal's same calls on a stored [R, d^2] table in the same run -- the floor -- and (b) the
  reference's operation sequence F.linear(B[p], W) + bmm + mm in torch on the same GPU.

HIP events around `--iters` calls after a warm-up call, median (min .. max) of `--repeats` windows, in microseconds per
call.  Reads nothing outside the tree.  Writes profiles/tucker3_probe.txt."""
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
        out.append(1e3 * a.elapsed_time(b) / iters)
    return float(np.median(out)), min(out), max(out)


def fmt(t):
    return f"{t[0]:8.1f} ({t[1]:.1f} .. {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=237)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--negatives", type=int, default=256)
    ap.add_argument("--base-dim", type=int, default=100)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tucker3_probe.txt"))
    args = ap.parse_args()
    from kge_amd import engine, model
    E, R, n, K, dr = args.entities, args.relations, args.n, args.negatives, args.base_dim
    lines = [f"tucker3_probe: E={E} R={R} n={n} K={K} d_r={dr} float32, us per call: median (min .. max) of {args.repeats} "
             f"windows of {args.iters} calls; {torch.cuda.get_device_name(0)}"]
    T = lambda fn: timed(fn, args.iters, args.repeats)  # noqa: E731
    for d in args.dims:
        torch.manual_seed(0)
        m = model.create("relational_tucker3", E, R, d, rel_base_dim=dr, device=DEV)
        with torch.no_grad():
            m._entity_embedder.weight.mul_(0.3)
            m._relation_embedder.projection.weight.mul_(0.03)
        r = model.create("rescal", E, R, d, device=DEV)
        B, W = m._bw()
        ent = m._entity_embedder.weight
        with torch.no_grad():
            r._entity_embedder.weight.copy_(ent)
            r._relation_embedder.weight.copy_(engine.tucker3_project(B, W))
        g = torch.Generator().manual_seed(1)
        s, p, o = (torch.randint(0, hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
        neg = torch.randint(0, E, (n, K), generator=g).to(DEV)
        gout = {"sp": torch.randn(n, E, generator=g).to(DEV), "sp_po": torch.randn(n, 2 * E, generator=g).to(DEV),
                "neg": torch.randn(n, K, generator=g).to(DEV)}
        with torch.no_grad():
            Bd, Wd = B.detach(), W.detach()
            t_all = T(lambda: engine.tucker3_project(Bd, Wd))
            t_rows = T(lambda: engine.tucker3_project(Bd, Wd, p))
            g_rows = torch.randn(n, d * d, generator=g).to(DEV)
            t_bwd = T(lambda: engine.tucker3_project_bwd(Bd, Wd, p, g_rows))
        lines.append(f"d={d}:")
        for name, t, rows in (("all R", t_all, R), ("gathered n", t_rows, n)):
            floor = rows * d * d * 4 / 8e12 * 1e6
            lines.append(f"  kge_tucker3_project {name:10s} {fmt(t)}   {rows * d * d * 4 / 1e6:.1f} MB written: "
                         f"{floor:.1f} us at 8 TB/s, {rows * d * d * 4 / t[0] / 1e6:.2f} TB/s reached")
        lines.append(f"  kge_tucker3_project_bwd (n rows) {fmt(t_bwd)}")

        def call(mm, kind, route=None):
            kw = {} if route is None else {"project": route}
            if kind == "sp":
                return mm.score_sp(s, p, **kw)
            if kind == "sp_po":
                return mm.score_sp_po(s, p, o, **kw)
            return mm.score_neg(s, p, o, 2, neg, **kw)

        def fwd_bwd(mm, kind, route=None):
            for prm in mm.parameters():
                prm.grad = None
            (call(mm, kind, route) * gout[kind]).sum().backward()

        def ref_call(kind):  # the reference's operation sequence
            M = torch.nn.functional.linear(B[p], W).view(-1, d, d)
            if kind == "neg":
                return (ent[s].unsqueeze(1).bmm(M).view(-1, 1, d) * ent[neg]).sum(-1)
            sp = ent[s].unsqueeze(1).bmm(M).view(-1, d).mm(ent.t())
            if kind == "sp":
                return sp
            return torch.cat((sp, M.bmm(ent[o].unsqueeze(2)).view(-1, d).mm(ent.t())), 1)

        def ref_fwd_bwd(kind):
            for prm in m.parameters():
                prm.grad = None
            (ref_call(kind) * gout[kind]).sum().backward()

        for kind in ("sp", "sp_po", "neg"):
            row = {}
            for route in ("all", "batch"):
                row[route, "fwd+bwd"] = T(lambda: fwd_bwd(m, kind, route))
                with torch.no_grad():
                    row[route, "fwd"] = T(lambda: call(m, kind, route))
            row["rescal", "fwd+bwd"] = T(lambda: fwd_bwd(r, kind))
            row["torch", "fwd+bwd"] = T(lambda: ref_fwd_bwd(kind))
            with torch.no_grad():
                row["rescal", "fwd"] = T(lambda: call(r, kind))
                row["torch", "fwd"] = T(lambda: ref_call(kind))
                err = float((call(m, kind, "batch") - ref_call(kind)).abs().max())
            for what in ("fwd", "fwd+bwd"):
                note = " (no-grad: the cached table)" if what == "fwd" else ""
                lines.append(f"  score_{kind:5s} {what:7s} all {fmt(row['all', what])}{note}   batch {fmt(row['batch', what])}   "
                             f"hip_rescal floor {fmt(row['rescal', what])}   torch linear+bmm+mm {fmt(row['torch', what])}")
            lines.append(f"    max |difference| to the torch sequence {err:.2e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
