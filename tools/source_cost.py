#!/usr/bin/env python3
"""What particle sources and sinks add to the one-GPU step: python tools/source_cost.py [--n 256] [--steps 20] [--warmup 5] [--prof]

The scene is bench.py's 256^3 water_cube_drop at 8 per cell.  Five fresh runs of the same steps: plain; a FILL source of
32 x 8 x 32 cells at 8 per cell above the pool (its new water adds its own work to every later phase: a taller active box, more
unknowns); "idle", the same source inside the falling cube, where it finds every cell full and emits nothing (the cost of the
source itself); a sink slab at the floor (y index 2..3: nothing reaches it in the first steps, so it measures the count pass
alone); both.  Each prints ms/step and the difference to the plain run.
--prof: the "both" run again under `rocprofv3 --kernel-trace --stats` (a child process) and the mean time of every
source / sink kernel from its trace."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("plain", "source", "idle", "sink", "both")
NEW_KERNELS = ("k_src_count", "k_src_plan", "k_src_emit", "k_interp_from_grid", "k_sink_mark", "k_sink_compact")


def run(fs, n, mode, steps, warmup):
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 8, seed=0))
    c = n // 2
    if mode in ("source", "both"):
        sim.set_source(0, (c - 16, n - 56, c - 16), (c + 15, n - 49, c + 15), 8, mode="fill", every=1, seed=1)
    if mode == "idle":   # the same FILL source inside the pool, where every cell already holds 8: the planning passes alone
        sim.set_source(0, (c - 16, c - 4, c - 16), (c + 15, c + 3, c + 15), 8, mode="fill", every=1, seed=1)
    if mode in ("sink", "both"):
        sim.set_sink(0, (2, 2, 2), (n - 3, 3, n - 3))
    for _ in range(warmup):
        sim.step()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ss = sim.source_stats()
    out = {"mode": mode, "ms_per_step": ms, "particles": sim.num_particles, "emitted_total": ss["emitted_total"],
           "removed_total": ss["removed_total"]}
    sim.close()
    return out


def kernel_times(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    acc = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("void ", "").replace("fl::", ""))
            if name in NEW_KERNELS:
                a = acc.setdefault(name, [0, 0])
                a[0] += 1
                a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return {k: {"launches": v[0], "mean_us": v[1] / v[0] / 1e3} for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=MODES)
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    res = {}
    for m in ([a.only] if a.only else MODES):
        res[m] = run(fs, a.n, m, a.steps, a.warmup)
        r = res[m]
        extra = ""
        if m != "plain" and "plain" in res:
            d = r["ms_per_step"] - res["plain"]["ms_per_step"]
            r["added_ms"] = d
            extra = f"  added {d * 1e3:+.0f} us/step ({100 * d / res['plain']['ms_per_step']:+.1f} %)"
        print(f"{m:7s} {r['ms_per_step']:.3f} ms/step  particles {r['particles']}  emitted {r['emitted_total']}  "
              f"removed {r['removed_total']}{extra}", flush=True)
    if a.prof:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--n", str(a.n), "--steps", str(a.steps), "--warmup", str(a.warmup), "--only", "both"]
            subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
            res["kernels"] = kernel_times(d)
        for k, v in sorted(res["kernels"].items()):
            print(f"{k:20s} {v['launches']:5d} launches  {v['mean_us']:8.2f} us mean")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
