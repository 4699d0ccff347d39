#!/usr/bin/env python3
"""The split-query group launch of the bench (8 two-sided batches, FB15k-237 shape, ComplEx d = 512, the bench's random
tables) on both shapes of the matrix instruction, switch V8_MFMA32 = 1 (v_mfma_f32_32x32x16_bf16) against the default
(v_mfma_f32_16x16x32_bf16):

  * interleaved rounds in ONE process (--rounds, default 5): per round and arm the bench's own region -- 2,000 steps =
    250 group launches, each building the next group's queries, behind the bench's warm-up floor -- timed by the host
    clock around a synchronise; median and minimum us per step of each arm;
  * the in-kernel clock of each arm (a -DKGE_V8_PROBES build only: the production kernel executes no stamp): after
    >= 2 s of back-to-back launches one launch stamps s_memtime and s_memrealtime per workgroup before its first chain
    and behind its last store (slots 48 - 51 of the debug buffer); clock = median over the workgroups of
    d(memtime) / d(memrealtime) x 100 MHz.

    python tools/v8_clock_probe.py [--lib PATH/libkge_amd.so] [--rounds N] [--seconds S]

--lib: a library built elsewhere (make -C <copy of kge_amd/csrc> CXXEXTRA=-DKGE_V8_PROBES), through the ctypes binding."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--seconds", type=float, default=2.0)
a = ap.parse_args()
if a.lib:
    os.environ["KGE_AMD_BINDING"] = "ctypes"  # (the torch extension is linked to the in-tree library)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kge_amd import _lib  # noqa: E402
if a.lib:
    _lib.LIB_PATH = os.path.abspath(a.lib)
from kge_amd import engine  # noqa: E402

dev = torch.device("cuda", 0)
E, R, D, n, L = 14541, 237, 512, 512, 8
WARMUP_MIN_STEPS = 8192  # bench.py's floor
P = engine.score_pitch(E)
ent = torch.empty(E, D).normal_(0, 0.1, generator=torch.Generator().manual_seed(0)).bfloat16().to(dev)
rel = torch.empty(R, D).normal_(0, 0.1, generator=torch.Generator().manual_seed(1234)).bfloat16().to(dev)
fl = engine.FLAG_SPLIT_QUERY
T = engine.Tables("complex", ent, rel, flags=fl)
q = torch.Generator().manual_seed(100 + L)
tri = [torch.stack([torch.randint(hi, (n * L,), generator=q) for hi in (E, R, E)], 1).to(dev) for _ in range(2)]
qs = [engine.QueriesGroup(T, "sp_po", n, L, flags=fl) for _ in range(2)]
engine.build_queries_group(T, "sp_po", tri[0], n, L, out=qs[0])
buf = torch.empty(L, n, 2 * P, device=dev)
out = buf.view(L, n, 2, P)[:, :, :, :E]
cur = [0]


def launch():
    c = cur[0]
    engine.score_queries_group(T, qs[c], out, next_batch=tri[1 - c], next_queries=qs[1 - c])
    cur[0] = 1 - c


ARMS = (("32x32x16", 1), ("16x16x32", None))
lib = _lib.lib()
lib.kge_debug_v6_stamps.restype = None
lib.kge_debug_v6_stamps.argtypes = [ctypes.c_void_p]

for _ in range(WARMUP_MIN_STEPS // L):
    launch()
torch.cuda.synchronize()

regions = {name: [] for name, _ in ARMS}
for rnd in range(a.rounds):
    for name, val in ARMS:
        _lib.set_switch("V8_MFMA32", val)
        for _ in range(8):
            launch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps // L):
            launch()
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / a.steps * 1e6
        regions[name].append(us)
        print(json.dumps({"round": rnd, "arm": name, "us_per_step": round(us, 3)}), flush=True)

clock = {}
for name, val in ARMS:
    _lib.set_switch("V8_MFMA32", val)
    st = torch.zeros(4096 * 64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        for _ in range(64):
            launch()
        torch.cuda.synchronize()  # (bounds the queue; 64 launches = ~15 ms between two of these)
    for _ in range(64):
        launch()
    lib.kge_debug_v6_stamps(ctypes.c_void_p(st.data_ptr()))
    launch()
    lib.kge_debug_v6_stamps(None)
    torch.cuda.synchronize()
    v = st.view(4096, 64).cpu()
    v = v[(v[:, 48] != 0) & (v[:, 50] != 0)]
    if v.shape[0] == 0:
        clock[name] = None  # not a probe build
        continue
    cyc = (v[:, 50] - v[:, 48]).double()
    ticks = (v[:, 51] - v[:, 49]).double()
    mhz = cyc / ticks * 100.0
    clock[name] = {"workgroups": int(v.shape[0]), "median_mhz": round(float(mhz.median()), 1),
                   "min_mhz": round(float(mhz.min()), 1), "max_mhz": round(float(mhz.max()), 1),
                   "median_cycles": int(cyc.median()), "median_us": round(float(ticks.median()) / 100.0, 2)}
_lib.set_switch("V8_MFMA32", None)

res = {"probe_build": clock["32x32x16"] is not None, "rounds": a.rounds, "steps_per_region": a.steps}
for name, _ in ARMS:
    r = regions[name]
    res[name] = {"us_per_step_median": round(statistics.median(r), 3), "us_per_step_min": round(min(r), 3),
                 "us_per_step_max": round(max(r), 3), "in_kernel_clock": clock[name]}
old, new = res["32x32x16"], res["16x16x32"]
res["median_ratio_32_over_16"] = round(old["us_per_step_median"] / new["us_per_step_median"], 4)
res["new_median_beats_old_fastest"] = new["us_per_step_median"] < old["us_per_step_min"]
print(json.dumps(res), flush=True)
