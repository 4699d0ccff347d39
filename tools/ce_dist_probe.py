"""Fused against composed 1vsAll step for TransE / RotatE (kge_amd.model, fused_dist_loss on / off): time per step and
torch.cuda.max_memory_allocated, l_norm 1 and 2, at E = 14,541 (FB15k-237) and E = 574,311 (a one-eighth Wikidata5M
shard), n = 512, d = 128.  --mode kvsall_kl / kvsall_bce: the KvsAll step instead (kl_loss_sp + kl_loss_po or
bce_loss_sp + bce_loss_po, no label smoothing) with 0..16 (about 8) random labels per row.  --mode f32_1vsall: the
1vsAll step of float32 ComplEx / DistMult with fused_f32_loss on / off (kge_ce_f32_*).  --mode f32_kvsall_kl /
f32_kvsall_bce: their KvsAll step (kge_kl_f32_* / kge_bce_f32_*) with the same label sets.

    python tools/ce_dist_probe.py [--mode 1vsall] [--out profiles/ce_dist_probe.txt] [--steps 10] [--limit 120]
    python tools/ce_dist_probe.py --mode kvsall_kl --out profiles/multilabel_dist_probe_kl.txt
    python tools/ce_dist_probe.py --mode f32_1vsall --out profiles/ce_f32_probe.txt
    python tools/ce_dist_probe.py --mode f32_kvsall_kl --out profiles/ml_f32_probe.txt

The parent never touches the GPU: every (shape, scorer, norm, path) step runs in a child process of its own under its
own time limit, and after a child that fails in any way other than running out of memory nothing more is started."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(14541, 237, 512, 128), (574311, 822, 512, 128)]


def one(name, l_norm, E, R, n, d, fused, steps, mode="1vsall"):
    import torch
    sys.path.insert(0, ROOT)
    from kge_amd import model as km
    dev = "cuda:0"
    torch.manual_seed(0)
    opt = {"fused_f32_loss": fused} if mode.startswith("f32_") else {"fused_dist_loss": fused}
    m = km.create(name, E, R, d, l_norm=l_norm, device=dev, **opt).train()
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(dev) for hi in (E, R, E))

    csr = []
    for _ in range(2 if "kvsall" in mode else 0):  # label CSRs of the sp_ and the _po queries: 0..16 labels per row
        k = torch.randint(0, 17, (n,), generator=g)
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(k, 0)
        col = torch.cat([torch.randperm(E, generator=g)[:int(x)] for x in k])
        csr.append((rowptr.to(dev), col.to(dev)))

    def step():
        m.zero_grad(set_to_none=True)
        if mode in ("1vsall", "f32_1vsall"):
            (m.loss_sp(s, p, o).sum() / n).backward()
            (m.loss_po(p, o, s).sum() / n).backward()
        elif mode in ("kvsall_kl", "f32_kvsall_kl"):
            (m.kl_loss_sp(s, p, *csr[0]).sum() / n).backward()
            (m.kl_loss_po(p, o, *csr[1]).sum() / n).backward()
        else:
            (m.bce_loss_sp(s, p, *csr[0]).sum() / n).backward()
            (m.bce_loss_po(p, o, *csr[1]).sum() / n).backward()

    try:
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            step()
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps({"ms_per_step": t0.elapsed_time(t1) / steps,
                          "peak_mb": torch.cuda.max_memory_allocated() / 2**20}))
    except torch.OutOfMemoryError:
        print(json.dumps({"oom": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="1vsall", choices=("1vsall", "kvsall_kl", "kvsall_bce", "f32_1vsall", "f32_kvsall_kl", "f32_kvsall_bce"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    ap.add_argument("--one", nargs=7, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        name, l_norm, E, R, n, d, fused = a.one
        return one(name, float(l_norm), int(E), int(R), int(n), int(d), fused == "1", a.steps, a.mode)
    f32 = a.mode.startswith("f32_")
    lines = [f"# fused ({'fused_f32_loss' if f32 else 'fused_dist_loss'}=True) against composed {a.mode} step, both "
             f"directions, n and d below; {a.steps} timed steps after one warm-up",
             "scorer l_norm E n d path ms_per_step peak_MB"]
    for E, R, n, d in SHAPES:
        for name in (("complex", "distmult") if f32 else ("transe", "rotate")):
            for l_norm in ((1,) if f32 else (1, 2)):  # (ComplEx / DistMult have no norm)
                for fused in (1, 0):
                    cmd = [sys.executable, os.path.abspath(__file__), "--mode", a.mode, "--steps", str(a.steps), "--one", name, str(l_norm),
                           str(E), str(R), str(n), str(d), str(fused)]
                    try:
                        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                    except subprocess.TimeoutExpired:
                        lines.append(f"{name} {l_norm} {E} {n} {d} {'fused' if fused else 'composed'} TIME-LIMIT -")
                        print("\n".join(lines[-1:]), "-- stopping: a step hit its time limit")
                        return finish(lines, a.out, 1)
                    if r.returncode != 0:
                        lines.append(f"{name} {l_norm} {E} {n} {d} {'fused' if fused else 'composed'} FAILED({r.returncode}) -")
                        print(r.stderr[-2000:])
                        return finish(lines, a.out, 1)
                    res = json.loads(r.stdout.strip().splitlines()[-1])
                    cell = "out-of-memory -" if res.get("oom") else f"{res['ms_per_step']:.3f} {res['peak_mb']:.0f}"
                    lines.append(f"{name} {l_norm} {E} {n} {d} {'fused' if fused else 'composed'} {cell}")
                    print(lines[-1], flush=True)
    return finish(lines, a.out, 0)


def finish(lines, out, rc):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
