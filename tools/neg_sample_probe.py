#!/usr/bin/env python
"""Per-batch time of drawing a negative-sampling batch's samples for the subject and the object slot, n = 512 positives
and K = 1000 samples per slot on an FB15k-237-sized vocabulary (14,541 entities, 237 relations, 272,115 synthetic
training triples), uniform and frequency sampling, with and without filtering against the training split:

  host     the reference's KgeSampler.sample for S and O on the host (kge/util/sampler.py:80-137, with filtering
           _filter_and_resample*, :163-196, 700-752) plus the copy of the two [n, K] int64 blocks to the device
           (train_negative_sampling.py:86-101) -- wall clock, the device idle before and synchronised after
  device   DeviceSampler.sample for both slots (kge_neg_sample, one launch per slot), HIP events around `--iters`
           calls, median and spread (min .. max) of `--repeats` windows

The host figure depends on how the reference's filter loop runs on the box: with numba it is compiled, with the
test harness's numba stand-in (oracle/ref_stubs) it is plain Python -- the header line says which.  Needs the
reference package (oracle/ref_harness.py finds it)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

S, P, O = 0, 1, 2


def host_sampler(folder, sampling_type, filtered):
    import ref_harness as rh
    rh.import_reference()
    from kge import Config, Dataset
    from kge.util import KgeSampler
    if sampling_type == "frequency" and not hasattr(torch, "_multinomial_alias_setup"):
        # the two private torch functions the reference's frequency sampler calls are gone from recent releases: stand-ins
        # with their contract, for the HOST leg only
        from kge_amd.sampler import alias_setup

        def setup(probs):
            q, J = alias_setup(probs.numpy())
            return torch.from_numpy(J), torch.from_numpy(q.astype(np.float64))

        def draw(q, J, n):
            bucket = torch.randint(len(q), (n,))
            return torch.where(torch.rand(n, dtype=q.dtype) < q[bucket], bucket, J[bucket])
        torch._multinomial_alias_setup, torch._multinomial_alias_draw = setup, draw
    config = Config()
    config.folder = tempfile.mkdtemp(prefix="neg_sample_probe_")
    config.set("console.quiet", True)
    config.set("dataset.name", "probe")
    config.set("negative_sampling.sampling_type", sampling_type)
    config.set("negative_sampling.implementation", "batch")  # (what the job makes of "auto" at K > 30; the draw ignores it)
    config.set("negative_sampling.filtering.s", filtered)
    config.set("negative_sampling.filtering.o", filtered)
    dataset = Dataset.create(config, folder=folder)
    return KgeSampler.create(config, "negative_sampling", dataset), dataset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-batches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neg_sample_probe.txt"))
    args = ap.parse_args()
    import ref_harness as rh
    rh.import_reference()  # (puts the reference package -- and, where numba is missing, its stand-in -- on the path)
    import numba
    from kge_amd import DeviceSampler
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    dev = torch.device("cuda", 0)
    E, R, N = 14541, 237, 272115
    root = tempfile.mkdtemp(prefix="neg_sample_probe_data_")
    splits = make_splits(E, R, N, 1024, 1024, seed=1)
    folder = write_libkge_dataset(os.path.join(root, "probe"), "probe", E, R, splits)
    compiled = "stand-in (plain Python loop)" if "ref_stubs" in (getattr(numba, "__file__", "") or "") else "compiled"
    lines = [f"# neg_sample_probe: n = {args.n}, K = {args.K} per slot, slots S + O, {E} entities, {R} relations, {N} training "
             f"triples; host: wall clock of {args.host_batches} batches, median (min .. max), numba {compiled}; device: HIP "
             f"events, median (min .. max) of {args.repeats} windows of {args.iters} batches; {torch.cuda.get_device_name(0)}",
             f"# {'sampling':<10}{'filtered':<10}{'host sample + copy, us':>34}{'device sampler, us':>34}{'host / device':>16}"]
    for sampling_type in ("uniform", "frequency"):
        for filtered in (False, True):
            sampler, dataset = host_sampler(folder, sampling_type, filtered)
            train = dataset.split("train")
            rng = np.random.default_rng(0)
            batches = [train[torch.from_numpy(rng.integers(0, len(train), args.n))].long() for _ in range(args.host_batches + 1)]
            host = []
            for k, tri in enumerate(batches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                blocks = [sampler.sample(tri, slot, args.K).to(dev) for slot in (S, O)]
                torch.cuda.synchronize()
                if k:  # (the first batch warms the index and the allocator)
                    host.append((time.perf_counter() - t0) * 1e6)
            del blocks
            ds = DeviceSampler(train, E, R, sampling_type=sampling_type, smoothing=1.0, filter_s=filtered, filter_o=filtered,
                               seed=1, device=dev)
            tri = batches[0].to(dev)

            def draw():
                ds.sample(tri, S, args.K)
                ds.sample(tri, O, args.K)
            for _ in range(5):
                draw()
            torch.cuda.synchronize()
            device = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    draw()
                b.record()
                b.synchronize()
                device.append(a.elapsed_time(b) / args.iters * 1e3)
            rejected = int(ds.last_stats[:, 0].sum()) if filtered else 0
            capped = int(ds.last_stats[:, 1].sum()) if filtered else 0
            h, d = np.median(host), np.median(device)
            lines.append(f"  {sampling_type:<10}{str(filtered):<10}{h:>12.1f} ({min(host):>9.1f} .. {max(host):>9.1f})"
                         f"{d:>12.1f} ({min(device):>7.1f} .. {max(device):>7.1f}){h / d:>15.1f}x"
                         f"   # last O block: {rejected} rejected draws, {capped} capped")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
