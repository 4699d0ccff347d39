#!/usr/bin/env python3
"""The tail of the split-query group launch of the bench (8 two-sided batches, FB15k-237 shape, ComplEx d = 512, the
bench's random tables; each launch builds the next group's queries): what lies between a workgroup's last score store
and the end of the launch, with the next group's build in CLAIMED slices (default) against one FIXED slice per workgroup
(switch V8_TAIL_FIXED = 1, the kernel before DESIGN 37):

  * interleaved rounds in ONE process (--rounds, default 7): per round and arm the bench's own region -- 2,000 steps =
    250 group launches behind the bench's warm-up floor -- timed by the host clock around a synchronise;
  * the tail of each arm (a -DKGE_V8_PROBES build only: the production kernel executes no stamp): after >= 2 s of
    back-to-back launches, --launches (default 9) stamped launches, 64 unstamped ones between two of them.  A stamped
    launch records s_memrealtime (100 MHz, one time base for the chip) per workgroup in front of its first chain (slot
    49), behind its last store (51) and behind its build, wave 0's stores acknowledged (53), and the slices it built
    (54).  Per launch: the spread of `last store` over the workgroups, the time from a workgroup's last store to its
    build done, the distance from the latest `last store` to the latest `build done`; reported as medians over the
    launches.

    python tools/v8_tail_probe.py [--lib PATH/libkge_amd.so] [--rounds N] [--launches K] [--seconds S]

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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--launches", type=int, default=9)
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


ARMS = (("fixed", 1), ("claimed", None))
lib = _lib.lib()
lib.kge_debug_v6_stamps.restype = None
lib.kge_debug_v6_stamps.argtypes = [ctypes.c_void_p]

for _ in range(WARMUP_MIN_STEPS // L):
    launch()
torch.cuda.synchronize()

regions = {name: [] for name, _ in ARMS}
for rnd in range(a.rounds):
    for name, val in ARMS:
        _lib.set_switch("V8_TAIL_FIXED", val)
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


def med(xs):
    return round(statistics.median(xs), 2)


tail = {}
for name, val in ARMS:
    _lib.set_switch("V8_TAIL_FIXED", val)
    st = torch.zeros(4096 * 64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        for _ in range(64):
            launch()
        torch.cuda.synchronize()  # (bounds the queue; 64 launches = ~15 ms between two of these)
    per = []
    for k in range(a.launches):
        for _ in range(64):
            launch()
        st.zero_()
        lib.kge_debug_v6_stamps(ctypes.c_void_p(st.data_ptr()))
        launch()
        lib.kge_debug_v6_stamps(None)
        torch.cuda.synchronize()
        v = st.view(4096, 64).cpu()
        v = v[(v[:, 51] != 0) & (v[:, 53] != 0)]
        if v.shape[0] == 0:
            break  # not a probe build
        start, last, done = (v[:, c].double() / 100.0 for c in (49, 51, 53))  # us
        built = v[:, 54]
        late = int(last.argmax())
        per.append({"workgroups": int(v.shape[0]),
                    "last_store_spread_us": float(last.max() - last.min()),
                    "build_per_workgroup_median_us": float((done - last).median()),
                    "build_per_workgroup_max_us": float((done - last).max()),
                    "latest_last_store_to_latest_build_done_us": float(done.max() - last.max()),
                    "first_start_to_latest_build_done_us": float(done.max() - start.min()),
                    "first_start_to_latest_last_store_us": float(last.max() - start.min()),
                    "slices_built_max": int(built.max()), "slices_built_by_latest_finisher": int(built[late])})
        print(json.dumps({"arm": name, "stamped_launch": k, **{kk: round(vv, 2) for kk, vv in per[-1].items()}}), flush=True)
    tail[name] = {k: med([p[k] for p in per]) for k in per[0]} if per else None
_lib.set_switch("V8_TAIL_FIXED", None)

res = {"probe_build": tail["fixed"] is not None, "rounds": a.rounds, "steps_per_region": a.steps,
       "stamped_launches": a.launches}
for name, _ in ARMS:
    r = regions[name]
    res[name] = {"us_per_step_median": round(statistics.median(r), 3), "us_per_step_min": round(min(r), 3),
                 "us_per_step_max": round(max(r), 3), "tail_medians": tail[name]}
old, new = res["fixed"], res["claimed"]
res["median_ratio_fixed_over_claimed"] = round(old["us_per_step_median"] / new["us_per_step_median"], 4)
res["claimed_slowest_beats_fixed_fastest"] = new["us_per_step_max"] < old["us_per_step_min"]
print(json.dumps(res), flush=True)
