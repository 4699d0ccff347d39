#!/usr/bin/env python
"""Forward + backward of ONE slot's block of shared negative samples (negative_sampling.shared: true), timed through

  today   what hip_negative_sampling did before kge_score_neg_shared: TransE / RotatE (implementation "triple",
          transe.py:58-68) materialise the [n, K] samples and go through score_neg; ComplEx / DistMult score the unique
          subset with score_sp / score_po and index the matrix as DefaultSharedNegativeSample.score does
          (sampler.py:537-578, restated below)
  new     model.score_neg_shared (kge_score_neg_shared + kge_score_neg_shared_bwd_accum)

Written at the kge_amd.model level: it needs no reference package, and `--route today` runs on a checkout that does not
have the new entry points yet (the parent commit: point PYTHONPATH at it).  HIP events around `--iters` iterations, a
warm-up first, `--repeats` such windows: the median and the spread (min .. max) of the per-iteration time are printed,
one line per case, and appended to --out.  Default sampling type (one spare id, one drop index per positive).
"""
import argparse
import os
import sys

import torch

try:  # (a PYTHONPATH that already holds a kge_amd -- the checkout to measure -- wins over this tree)
    import kge_amd  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def materialise(unique, drop, repeat, n):
    """DefaultSharedNegativeSample.samples (sampler.py:503-535) without the host wait of its torch.nonzero."""
    uc = unique.numel() - 1
    hit = torch.arange(uc, device=unique.device).unsqueeze(0) == drop.unsqueeze(1)
    neg = torch.where(hit, unique[uc], unique[:uc].unsqueeze(0).expand(n, -1))
    if repeat.numel():
        neg = torch.cat([neg, neg[:, repeat]], dim=1)
    return neg.contiguous()


def sampler_indexing(all_scores, drop, repeat):
    """DefaultSharedNegativeSample.score after _score_unique_targets (sampler.py:551-576), op for op."""
    n, uc = all_scores.shape[0], all_scores.shape[1] - 1
    drop_rows = torch.nonzero(drop != uc, as_tuple=False).squeeze()
    scores = torch.empty(n, uc, device=all_scores.device)
    scores[:, :] = all_scores[:, :-1]
    scores[drop_rows, drop[drop_rows]] = all_scores[drop_rows, -1]
    if repeat.numel():
        scores = scores[:, torch.cat((torch.arange(uc, device=scores.device), repeat))]
    return scores


def block(m, name, route, slot, s, p, o, unique, drop, repeat):
    if route == "new":
        return m.score_neg_shared(s, p, o, slot, unique, drop, repeat)
    if name in ("transe", "rotate"):
        return m.score_neg(s, p, o, slot, materialise(unique, drop, repeat, s.numel()))
    all_scores = m.score_po(p, o, unique) if slot == 0 else m.score_sp(s, p, unique)
    return sampler_indexing(all_scores, drop, repeat)


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
        out.append(a.elapsed_time(b) / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["today", "new", "both"], default="both")
    ap.add_argument("--scorers", default="transe,rotate,complex,distmult")
    ap.add_argument("--shapes", default="14541:512:100,14541:512:1000,4594485:1024:1000", help="E:n:K,...")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neg_shared_probe: no GPU (a timing needs one)")
    from kge_amd import model
    lines_head = f"# {args.tag}: kge_amd from {os.path.relpath(os.path.dirname(os.path.abspath(model.__file__)))}"
    dev = torch.device("cuda", 0)
    lines = [lines_head]
    for shape in args.shapes.split(","):
        E, n, K = (int(x) for x in shape.split(":"))
        for name in args.scorers.split(","):
            try:
                torch.manual_seed(0)
                m = model.create(name, E, 50, args.dim, device=dev).train()
            except torch.OutOfMemoryError:
                lines.append(f"{args.tag} {name} E={E}: tables do not fit")
                continue
            g = torch.Generator().manual_seed(1)
            s, p, o = (torch.randint(hi, (n,), generator=g).to(dev) for hi in (E, 50, E))
            # a sample as KgeUniformSampler._sample_shared draws it (sampler.py:620-698): K draws with replacement
            # leave Uc distinct ids, K - Uc repeats
            uc = int(torch.unique(torch.randint(E - 1, (K,), generator=g)).numel())
            unique = torch.randperm(E, generator=g)[:uc + 1].to(dev)
            drop = torch.randint(uc + 1, (n,), generator=g).to(dev)
            repeat = torch.randint(uc, (K - uc,), generator=g).to(dev)
            w = torch.randn(n, K, generator=g).to(dev)
            for route in (("today", "new") if args.route == "both" else (args.route,)):
                if route == "new" and not hasattr(m, "score_neg_shared"):
                    continue
                for slot in (0, 2):
                    def fwd():
                        with torch.no_grad():
                            return block(m, name, route, slot, s, p, o, unique, drop, repeat)

                    def fwd_bwd():
                        m.zero_grad(set_to_none=True)
                        (block(m, name, route, slot, s, p, o, unique, drop, repeat) * w).sum().backward()

                    f = timed(fwd, args.iters, args.repeats, args.warmup)
                    fb = timed(fwd_bwd, args.iters, args.repeats, args.warmup)
                    lines.append(f"{args.tag} {name:8s} E={E} d={args.dim} n={n} K={K} Uc={uc} slot={slot} route={route:5s} "
                                 f"fwd {f[0]:.4f} ms ({f[1]:.4f} .. {f[2]:.4f})  fwd+bwd {fb[0]:.4f} ms "
                                 f"({fb[1]:.4f} .. {fb[2]:.4f})")
                    print(lines[-1], flush=True)
            del m
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
