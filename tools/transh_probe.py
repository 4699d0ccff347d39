#!/usr/bin/env python
"""Time of the TransH scoring entry points at the FB15k-237 shape (E = 14,541, d = 128, n = 512), L1 and L2, beside

  (a) the TransE entry at the same shape and norm (same tables' entity rows, same run);
  (b) the reference's operation sequence (kge/model/transh.py:39-78: every target projected once per relation, an
      [m, n, d] tensor) in torch on the GPU, at n = 64 (the [m, n, d] tensor is 476 MB there), with the TransH entry at
      n = 64 beside it.

HIP events around `--iters` calls after a warm-up call, median (min .. max) of `--repeats` windows, in microseconds per
call; contiguous [n, m] outputs (padded=False).  Writes profiles/transh_probe.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
F = torch.nn.functional


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


def ref_sp(ent, rel, s, p, lp):
    d = ent.shape[1]
    pe = rel[p]
    r, w = pe[:, :d], F.normalize(pe[:, d:], p=2, dim=-1)
    n, m = pe.shape[0], ent.shape[0]
    se = ent[s]
    q = (se - torch.sum(se * w, dim=-1, keepdim=True) * w + r).repeat(m, 1)
    t, wm = ent.repeat_interleave(n, 0), w.repeat(m, 1)
    t = t - torch.sum(t * wm, dim=-1, keepdim=True) * wm
    return -F.pairwise_distance(q, t, p=lp).view(m, n).t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--n-ref", type=int, default=64)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transh_probe.txt"))
    args = ap.parse_args()
    from kge_amd import engine
    E, d, n = args.entities, args.dim, args.n
    g = torch.Generator().manual_seed(0)
    ent = (torch.randn(E, d, generator=g) * 0.3).to(DEV)
    rel_h = (torch.randn(237, 2 * d, generator=g) * 0.3).to(DEV)
    rel_e = rel_h[:, :d].contiguous()
    s = torch.randint(0, E, (n,), generator=g).to(DEV)
    p = torch.randint(0, 237, (n,), generator=g).to(DEV)
    o = torch.randint(0, E, (n,), generator=g).to(DEV)
    lines = [f"transh_probe: E={E} d={d} float32, us per call: median (min .. max) of {args.repeats} windows of "
             f"{args.iters} calls; {torch.cuda.get_device_name(0)}"]
    for lp in (1.0, 2.0):
        th = engine.Tables("transh", ent, rel_h, lp)
        te = engine.Tables("transe", ent, rel_e, lp)
        res = {}
        for name, t in (("transh", th), ("transe", te)):
            res[name, "sp"] = timed(lambda: engine.score_sp(t, s, p, padded=False), args.iters, args.repeats)
            res[name, "sp_po"] = timed(lambda: engine.score_sp_po(t, s, p, o), args.iters, args.repeats)
        lines.append(f"l_norm={lp:g} n={n}")
        for k in ("sp", "sp_po"):
            ratio = res["transh", k][0] / res["transe", k][0]
            lines.append(f"  score_{k:6s} transh {fmt(res['transh', k])}   transe {fmt(res['transe', k])}   ratio {ratio:.2f}")
        nr = args.n_ref
        sr, pr = s[:nr], p[:nr]
        got, want = engine.score_sp(th, sr, pr, padded=False), ref_sp(ent, rel_h, sr, pr, lp)
        err = float((got - want).abs().max())
        t_k = timed(lambda: engine.score_sp(th, sr, pr, padded=False), args.iters, args.repeats)
        t_r = timed(lambda: ref_sp(ent, rel_h, sr, pr, lp), max(2, args.iters // 5), args.repeats)
        lines.append(f"  n={nr}: score_sp transh {fmt(t_k)}   reference op sequence in torch {fmt(t_r)}   "
                     f"ratio {t_r[0] / t_k[0]:.1f}   max |difference| {err:.2e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
