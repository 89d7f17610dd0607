#!/usr/bin/env python3
"""What the liquid surface costs per step: python tools/sdf_cost.py [--n 256] [--ppc 8] [--steps 20] [--warmup 5] [--runs 3] [--late 0]
                                                                   [--radius 1.5] [--half-width 2.5] [--prof] [--visits]

Wall ms per step of the same steps in three forms, each in a fresh handle, `--runs` times:
  none     no output
  leaves   the density grid: fluid_output_snapshot after the step, fluid_output_wait one step later, a writer thread appends the
           leaf list to the step's own file and to the growing mygrids.vdb (tools/output_cost.py's `leaves`)
  surface  the level set of the particles: fluid_sdf_snapshot after the step, fluid_sdf_wait one step later, a writer thread
           writes surface<i>.vdb with fluid_write_vdb_sdf
The addends `leaves - none` and `surface - none` come from the same run of this script.  --late K: K steps without output first.
--prof: the `surface` form again under `rocprofv3 --kernel-trace --stats` (a child process): times of the k_sdf_* kernels and of the
scan they use.  --visits: the `surface` form again in a child with FLUID_SDF_VISITS=1: cells looked at per searched voxel."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("none", "leaves", "surface")


class Writer(threading.Thread):
    """One grid at a time, in step order; ctypes releases the GIL inside the library call."""

    def __init__(self, fs, n, d, stream):
        super().__init__(daemon=True)
        self.fs, self.n, self.d, self.stream = fs, n, d, stream
        self.cv = threading.Condition()
        self.job, self.done, self.quit, self.busy_s, self.file_bytes = None, 0, False, 0.0, 0

    def run(self):
        fs = self.fs
        while True:
            with self.cv:
                self.cv.wait_for(lambda: self.job is not None or self.quit)
                if self.job is None:
                    return
                i, g = self.job
            t0 = time.perf_counter()
            if self.stream is not None:
                path = os.path.join(self.d, f"mygrids{i}.vdb")
                w = fs.VdbStream(path, self.n, 1)
                hs = (C.c_void_p * 2)(w._h.value, self.stream._h.value)
                fs.check(fs.lib.fluid_vdb_append_leaves(hs, 2, C.byref(g)))
                w.close()
            else:
                path = os.path.join(self.d, f"surface{i}.vdb")
                fs.check(fs.lib.fluid_write_vdb_sdf(path.encode(), C.byref(g), 3))
                self.file_bytes += os.path.getsize(path)
            os.unlink(path)
            self.busy_s += time.perf_counter() - t0
            with self.cv:
                self.job, self.done = None, i + 1
                self.cv.notify_all()

    def wait_done(self, k):
        with self.cv:
            self.cv.wait_for(lambda: self.done >= k)

    def submit(self, i, g):
        with self.cv:
            self.cv.wait_for(lambda: self.job is None)
            self.job = (i, g)
            self.cv.notify_all()

    def stop(self):
        with self.cv:
            self.quit = True
            self.cv.notify_all()
        self.join()


def run(fs, a, mode):
    n, steps = a.n, a.steps
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, a.ppc, seed=0))
    for _ in range(a.late + a.warmup):
        sim.step()
    out = {"mode": mode}
    prm = fs.SdfParams(a.radius, a.half_width)
    with tempfile.TemporaryDirectory() as d:
        stream = fs.VdbStream(os.path.join(d, "mygrids.vdb"), n, steps) if mode == "leaves" else None
        wr = None
        if mode != "none":
            wr = Writer(fs, n, d, stream)
            wr.start()

        def wait():
            if mode == "leaves":
                g = fs.LeafGridC()
                fs.check(fs.lib.fluid_output_wait(sim._h, C.byref(g)))
            else:
                g = fs.SdfGridC()
                fs.check(fs.lib.fluid_sdf_wait(sim._h, C.byref(g)))
            return g
        listed, to_host = [], []
        t0 = time.perf_counter()
        for i in range(steps):
            sim.step()
            if mode == "none":
                continue
            wr.wait_done(i - 1)
            if mode == "leaves":
                sim.output_snapshot()
                st = sim.output_stats()
            else:
                fs.check(fs.lib.fluid_sdf_snapshot(sim._h, C.byref(prm)))
                st = sim.sdf_stats()
            listed.append(st["leaves_listed"]); to_host.append(st["bytes_to_host"])
            out["leaves_in_grid"] = st["leaves_in_grid"]
            if i > 0:
                wr.submit(i - 1, wait())
        if wr:
            wr.submit(steps - 1, wait())
            wr.wait_done(steps)
        out["ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
        if wr:
            wr.stop()
            out["writer_busy_ms_per_step"] = wr.busy_s / steps * 1e3
            out["leaves_listed_mean"] = sum(listed) / steps
            out["leaves_listed_max"] = max(listed)
            out["bytes_to_host_mean"] = sum(to_host) / steps
            if mode == "surface":
                out["file_bytes_mean"] = wr.file_bytes / steps
        if stream:
            stream.close()
    out["particles"] = sim.num_particles
    sim.close()
    return out


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"[<(].*", "", r["Kernel_Name"].replace("void ", "").replace("fl::", ""))
            if name.startswith("k_sdf_"):
                acc.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "mean_us": sum(v) / len(v), "min_us": min(v), "max_us": max(v)} for k, v in acc.items()}


def child_args(a):
    return [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--ppc", str(a.ppc), "--steps", str(a.steps), "--warmup", str(a.warmup),
            "--late", str(a.late), "--radius", str(a.radius), "--half-width", str(a.half_width), "--runs", "1", "--only", "surface"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--late", type=int, default=0)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--half-width", type=float, default=2.5)
    ap.add_argument("--only", choices=MODES)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--visits", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    res = {"n": a.n, "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "late": a.late, "radius": a.radius, "half_width": a.half_width,
           "runs": {m: [] for m in MODES}}
    for k in range(a.runs):
        for m in ([a.only] if a.only else MODES):
            r = run(fs, a, m)
            res["runs"][m].append(r)
            extra = ""
            if m != "none":
                extra = (f"  leaves {r['leaves_listed_mean']:.0f} / {r['leaves_in_grid']} (max {r['leaves_listed_max']})  "
                         f"to host {r['bytes_to_host_mean'] / 1e6:.2f} MB/step  writer busy {r['writer_busy_ms_per_step']:.2f} ms/step")
            print(f"n={a.n} late={a.late} run {k} {m:7s} {r['ms_per_step']:9.3f} ms/step{extra}", flush=True)
    ms = {m: [r["ms_per_step"] for r in v] for m, v in res["runs"].items() if v}
    if all(m in ms for m in MODES):
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        res["summary"] = {"median_ms": med, "none_spread_ms": max(ms["none"]) - min(ms["none"]), "leaves_minus_none_ms": med["leaves"] - med["none"],
                          "surface_minus_none_ms": med["surface"] - med["none"]}
        print(f"median ms/step: none {med['none']:.3f} (spread {res['summary']['none_spread_ms']:.3f})  leaves {med['leaves']:.3f}  surface {med['surface']:.3f}  "
              f"leaves - none {med['leaves'] - med['none']:+.3f}  surface - none {med['surface'] - med['none']:+.3f}", flush=True)
    if a.visits:
        r = subprocess.run(child_args(a), check=True, timeout=900, capture_output=True, text=True, env=dict(os.environ, FLUID_SDF_VISITS="1"))
        rows = [[float(x) for x in re.findall(r"[0-9.]+", ln)] for ln in r.stderr.splitlines() if ln.startswith("sdf visits:")]
        cells, searched, in_range = (sum(x[k] for x in rows) for k in range(3))
        res["visits"] = {"snapshots": len(rows), "cells_per_searched_voxel": cells / (512 * searched), "leaves_searched_mean": searched / len(rows),
                         "leaves_in_range_mean": in_range / len(rows)}
        print("visits:", json.dumps(res["visits"]), flush=True)
    if a.prof:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + child_args(a)
            subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
            res["kernels"] = kernel_times(d)
        for k, v in sorted(res["kernels"].items()):
            print(f"{k:14s} {v['launches']:5d} launches  mean {v['mean_us']:9.2f} us  min {v['min_us']:9.2f}  max {v['max_us']:9.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
