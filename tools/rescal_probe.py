#!/usr/bin/env python
"""Time of the RESCAL entry points at the FB15k-237 shape (E = 14,541, R = 237, n = 512) at d = 128 and d = 256, beside

  (a) float32 DistMult on the same entity table (the floor of the second stage: the same pair kernel without a build);
  (b) the reference's operation sequence (kge/model/rescal.py:36-42: bmm + mm) in torch on the same GPU.

HIP events around `--iters` calls after a warm-up call, median (min .. max) of `--repeats` windows, in microseconds per
call; contiguous [n, m] outputs (padded=False).  Writes profiles/rescal_probe.txt."""
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
    return f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f})"


def ref_sp(ent, rel, s, p):
    d = ent.shape[1]
    return ent[s].unsqueeze(1).bmm(rel[p].view(-1, d, d)).view(-1, d).mm(ent.t())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=237)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--negatives", type=int, default=256)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescal_probe.txt"))
    args = ap.parse_args()
    from kge_amd import engine
    E, R, n, K = args.entities, args.relations, args.n, args.negatives
    lines = [f"rescal_probe: E={E} R={R} n={n} K={K} float32, us per call: median (min .. max) of {args.repeats} windows of "
             f"{args.iters} calls; {torch.cuda.get_device_name(0)}"]
    for d in args.dims:
        g = torch.Generator().manual_seed(0)
        ent = (torch.randn(E, d, generator=g) * 0.3).to(DEV)
        rel = (torch.randn(R, d * d, generator=g) * 0.1).to(DEV)
        rel_d = (torch.randn(R, d, generator=g) * 0.3).to(DEV)
        s, p, o = (torch.randint(0, hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
        neg = torch.randint(0, E, (n, K), generator=g).to(DEV)
        tr, td = engine.Tables("rescal", ent, rel), engine.Tables("distmult", ent, rel_d)
        T = lambda fn: timed(fn, args.iters, args.repeats)
        q_sp = T(lambda: engine.rescal_queries(tr, "sp_", s, p))
        q_po = T(lambda: engine.rescal_queries(tr, "_po", o, p))
        res = {}
        for name, t in (("rescal", tr), ("distmult", td)):
            res[name, "sp"] = T(lambda: engine.score_sp(t, s, p, padded=False))
            res[name, "sp_po"] = T(lambda: engine.score_sp_po(t, s, p, o))
            res[name, "neg"] = T(lambda: engine.score_neg(t, s, p, o, 2, neg))
            gout = torch.randn(n, E, generator=torch.Generator().manual_seed(1)).to(DEV)
            res[name, "pairs_bwd"] = T(lambda: engine.score_pairs_bwd(t, "sp", s, p, None, gout))
            gneg = torch.randn(n, K, generator=torch.Generator().manual_seed(2)).to(DEV)
            ge, gr = torch.zeros_like(t.ent), torch.zeros_like(t.rel)
            res[name, "neg_bwd_accum"] = T(lambda: engine.score_neg_bwd_accum(t, s, p, o, 2, neg, gneg, None, ge, gr))
        got, want = engine.score_sp(tr, s, p, padded=False), ref_sp(ent, rel, s, p)
        err = float((got - want).abs().max())
        t_ref = T(lambda: ref_sp(ent, rel, s, p))
        lines.append(f"d={d}: the ungrouped build reads n d^2 floats = {n * d * d * 4 / 1e6:.1f} MB "
                     f"({R * d * d * 4 / 1e6:.1f} MB of distinct matrices)")
        lines.append(f"  kge_rescal_queries  sp_ {fmt(q_sp)}   _po {fmt(q_po)}")
        for k in ("sp", "sp_po", "neg", "pairs_bwd", "neg_bwd_accum"):
            a, b = res["rescal", k], res["distmult", k]
            lines.append(f"  {k:14s} rescal {fmt(a)}   distmult {fmt(b)}   ratio {a[0] / b[0]:.2f}")
        lines.append(f"  build share of kge_score_sp: {q_sp[0] / res['rescal', 'sp'][0]:.2f}")
        lines.append(f"  reference op sequence (bmm + mm) in torch, sp_: {fmt(t_ref)}   ratio to kge_score_sp "
                     f"{t_ref[0] / res['rescal', 'sp'][0]:.2f}   max |difference| {err:.2e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
