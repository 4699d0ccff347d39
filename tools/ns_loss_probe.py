#!/usr/bin/env python
"""Time per slot loss (forward + gradient of the scores) of LibKGE's negative-sampling losses kl / margin_ranking /
soft_margin / se on one [n, 1 + K] score block:

  torch    the reference's op sequence (kge/util/loss.py:192-274) in PyTorch-ROCm on the label matrix the job builds,
           torch autograd for the gradient -- what hip_negative_sampling runs with fused_other_losses: false
  kernel   the stand-in's route: engine.ns_loss (kge_ns_loss, one launch) + rows.sum() + the gradient's scaling
  parts    engine.ns_loss_parts on (pos [n], neg [n, K]) + the same: the captured step's form (no cat, no split)

Default shape n = 512, K = 1000 (BASELINE configs[2]).  HIP events around `--iters` iterations after a warm-up,
`--repeats` such windows: median and spread (min .. max) of the per-iteration time, one line per case, appended to
--out.  The torch route of margin_ranking holds two nonzero() calls = two host waits per iteration: its time is wall
clock of the device queue INCLUDING those waits, which is what a training step pays.  Needs no reference package."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

try:
    import kge_amd  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KINDS = ("kl", "margin_ranking", "soft_margin", "se")


def torch_loss(scores, labels, kind, margin):
    """kge/util/loss.py:211-213, 236-252, 221-224, 272-274, op for op."""
    if kind == "kl":
        return torch.nn.KLDivLoss(reduction="sum")(F.log_softmax(scores, dim=1), F.normalize(labels.float(), p=1, dim=1))
    if kind == "margin_ranking":
        K = scores.shape[1] - 1
        flat = labels.view(-1)
        pos_positives = flat.nonzero().view(-1)
        pos_negatives = (flat == 0).nonzero().view(-1)
        pos_positives = pos_positives.view(-1, 1).repeat(1, K).view(-1)
        positives = scores.view(-1)[pos_positives].view(-1)
        negatives = scores.view(-1)[pos_negatives].view(-1)
        target = torch.ones(positives.size()).to(scores.device)
        return torch.nn.MarginRankingLoss(margin=margin, reduction="sum")(positives, negatives, target)
    if kind == "soft_margin":
        return torch.nn.SoftMarginLoss(reduction="sum")(scores.view(-1), (labels * 2 - 1).view(-1))
    return torch.nn.MSELoss(reduction="sum")(scores, labels)


def timed(fn, iters, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kge_amd import engine
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    scores = (torch.randn(a.n, 1 + a.K, generator=g) * 4.0).to(dev)
    labels = torch.zeros(a.n, 1 + a.K, device=dev)
    labels[:, 0] = 1
    pos, neg = scores[:, 0].contiguous(), scores[:, 1:].contiguous()
    inv = torch.full((), 1.0 / a.n, device=dev)
    lines = [f"# ns_loss_probe: n = {a.n}, K = {a.K}, margin = {a.margin}; us per slot loss (forward + gradient), "
             f"median (min .. max) of {a.repeats} windows of {a.iters} iterations, HIP events; {torch.cuda.get_device_name(0)}",
             f"# {'kind':<16}{'torch op sequence':>28}{'kernel (block)':>28}{'kernel (parts)':>28}{'torch / block':>16}"]

    for kind in KINDS:
        arg = a.margin if kind == "margin_ranking" else 0.0

        def by_torch():
            x = scores.detach().requires_grad_(True)
            (torch_loss(x, labels, kind, a.margin) * inv).backward()
            return x.grad

        def by_kernel():
            rows, grad = engine.ns_loss(scores, kind, arg)
            return rows.sum() * inv, grad * inv

        def by_parts():
            rows, g_pos, g_neg = engine.ns_loss_parts(pos, neg, kind, arg)
            return rows.sum() * inv, g_pos * inv, g_neg * inv

        t, k, p = (timed(f, a.iters, a.repeats, a.warmup) for f in (by_torch, by_kernel, by_parts))
        fmt = lambda m: f"{m[0]:9.1f} ({m[1]:7.1f} ..{m[2]:8.1f})"
        lines.append(f"  {kind:<16}{fmt(t):>28}{fmt(k):>28}{fmt(p):>28}{t[0] / k[0]:>15.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
