#!/usr/bin/env python
"""Per-batch time of building a KvsAll batch at the FB15k-237 shape: n = 512 examples over both query types (sp_ and
_po) of a synthetic training split with the dataset's degree distribution (14,541 entities, 237 relations, 272,115
triples: kge_amd/synthetic.py), up to the padded inputs of the captured step:

  host     what a batch costs without hip_KvsAll.device_collate: the reference's collate closure
           (kge/job/train_KvsAll.py:118-201), the copy of queries / label_coords / query_type_indexes to the device, the
           per-type cut (_kvsall_per_type_cut) and the padding (_kvsall_pad_inputs) -- wall clock per batch, the device
           idle before and synchronised after
  device   DeviceKvsAllCollator: the copy of the example numbers, batch() and typed(caps) -- two kge_kvsall_collate
           calls, four launches -- HIP events around `--iters` batches, median and spread (min .. max) of `--repeats`
           windows (the window holds the collator's host work too: sizes, fit test, the calls); and the same loop on
           the wall clock

Needs the reference package (oracle/ref_harness.py finds it)."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-batches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kvsall_collate_probe.txt"))
    args = ap.parse_args()
    import ref_harness as rh
    rh.import_reference()
    from kge.indexing import KvsAllIndex
    from kge.job.train_KvsAll import TrainingJobKvsAll
    from kge_amd import DeviceKvsAllCollator
    from kge_amd.libkge_plugin.train_job import _kvsall_pad_inputs, _kvsall_per_type_cut
    from kge_amd.synthetic import make_splits
    dev = torch.device("cuda", 0)
    E, R, N = 14541, 237, 272115
    train = torch.from_numpy(np.asarray(make_splits(E, R, N, 1024, 1024, seed=1)["train"])).int()
    query_types = ["sp_", "_po"]
    indexes = [KvsAllIndex(train, [0, 1], 2, list), KvsAllIndex(train, [1, 2], 0, list)]
    last = list(np.cumsum([len(ix) for ix in indexes]))
    job = types.SimpleNamespace(query_types=query_types, query_indexes=indexes, query_last_example=last)
    collate = TrainingJobKvsAll._get_collate_fun(job)
    collator = DeviceKvsAllCollator(indexes, query_types, dev)
    rng = np.random.default_rng(0)
    batches = [rng.permutation(int(last[-1]))[:args.n].astype(np.int64) for _ in range(max(args.host_batches, args.iters) + 1)]
    sizes = [collator.sizes(b) for b in batches]
    rows_cap = (int(max(s[0].max() for s in sizes) * 1.15 + 16) + 31) // 32 * 32
    lab_cap = (int((max(s[1].max() for s in sizes) + rows_cap) * 1.5) + 255) // 256 * 256
    caps = (rows_cap, lab_cap)

    def host_batch(examples):
        b = collate([int(x) for x in examples])
        coords = b["label_coords"].to(dev)
        queries, qtype = b["queries"].to(dev), b["query_type_indexes"].to(dev)
        per_type, _ = _kvsall_per_type_cut(queries, coords, qtype, query_types, len(examples))
        return _kvsall_pad_inputs(per_type, len(examples), dev, caps)

    def device_batch(examples):
        ex = torch.from_numpy(examples)
        dev_ex = ex.to(dev)
        b = collator.batch(ex, device_examples=dev_ex)
        return b, collator.typed(ex, caps=caps, weight=1.0 / len(examples), device_examples=dev_ex)

    # the two paths build the same tensors
    want, (b, typed) = host_batch(batches[0]), device_batch(batches[0])
    assert want is not None and typed is not None
    for k, t in enumerate(typed):
        for x, y in zip(want[4 * k:4 * k + 4], t[:4]):
            assert torch.equal(x, y)
    host = []
    for k, examples in enumerate(batches[:args.host_batches + 1]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_batch(examples)
        torch.cuda.synchronize()
        if k:  # (the first batch warms the allocator)
            host.append((time.perf_counter() - t0) * 1e6)
    for examples in batches[:5]:
        device_batch(examples)
    torch.cuda.synchronize()
    events, wall = [], []
    for _ in range(args.repeats):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for examples in batches[:args.iters]:
            device_batch(examples)
        z.record()
        z.synchronize()
        wall.append((time.perf_counter() - t0) / args.iters * 1e6)
        events.append(a.elapsed_time(z) / args.iters * 1e3)
    # the kernels alone: one batch's four launches again and again, no host work in between
    ex = torch.from_numpy(batches[0])
    dev_ex = ex.to(dev)
    nnz = int(collator.sizes(ex)[1].sum())
    from kge_amd import engine
    kern = []
    for _ in range(args.repeats):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            engine.kvsall_collate(collator._types, dev_ex, nnz, batch=True)
            engine.kvsall_collate(collator._types, dev_ex, nnz, batch=False, caps=[caps, caps], weight=1.0 / args.n)
        z.record()
        z.synchronize()
        kern.append(a.elapsed_time(z) / args.iters * 1e3)
    h, d, w, kk = np.median(host), np.median(events), np.median(wall), np.median(kern)
    nnz_all = [int(s[1].sum()) for s in sizes]
    text = "\n".join([
        f"# kvsall_collate_probe: n = {args.n}, query types sp_ + _po, {E} entities, {R} relations, {N} training triples, "
        f"{int(last[-1])} examples; labels per batch {min(nnz_all)} .. {max(nnz_all)}; padded to {rows_cap} rows and "
        f"{lab_cap} label entries per type; {torch.cuda.get_device_name(0)}",
        f"# host: wall clock of {args.host_batches} batches, median (min .. max); device: HIP events and wall clock, median "
        f"(min .. max) of {args.repeats} windows of {args.iters} batches",
        f"  (a) host: reference collate + copies + per-type cut + padding, us   {h:>10.1f} ({min(host):>9.1f} .. {max(host):>9.1f})",
        f"  (b) device collator: batch() + typed(caps), HIP events, us          {d:>10.1f} ({min(events):>9.1f} .. {max(events):>9.1f})",
        f"      the same windows on the wall clock, us                          {w:>10.1f} ({min(wall):>9.1f} .. {max(wall):>9.1f})",
        f"      the two kge_kvsall_collate calls alone (one batch, no host work in between), us {kk:>8.1f} "
        f"({min(kern):>7.1f} .. {max(kern):>7.1f})",
        f"  (a) / (b)                                                           {h / d:>10.1f}x",
    ]) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
