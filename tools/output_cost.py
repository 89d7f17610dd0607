#!/usr/bin/env python3
"""What writing every step's density grid costs: python tools/output_cost.py [--n 256] [--ppc 8] [--steps 20] [--warmup 5] [--runs 3] [--late 0] [--prof]

Wall ms per step of the same steps in three forms, each in a fresh handle, `--runs` times:
  none     no output
  dense    fluid_download_field(OUTPUT) + fluid_write_vdb (the step's own file) + fluid_vdb_append (the growing mygrids.vdb),
           all on the stepping thread: the loop `FLUID_OUT_DENSE=1 ./run.sh fluid` keeps
  leaves   fluid_output_snapshot after the step, fluid_output_wait one step later, and a writer thread that hands the leaf
           list to fluid_vdb_append_leaves for both files while the next step runs: the driver's default loop
--n 121 --ppc 10 is the reference's scene (its own scatter), any other n the scaled water_cube_drop.  --late K: K steps without
output first (the settled pool lists the most leaves).  Files go to a temporary directory.  The yardstick of `leaves` is `dense`
measured in the same run of this script on the same host.
--prof: the `leaves` form again under `rocprofv3 --kernel-trace --stats` (a child process) and the mean time of k_out_mark / k_out_pack."""
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

MODES = ("none", "dense", "leaves")
NEW_KERNELS = ("k_out_mark", "k_out_pack")


class Writer(threading.Thread):
    """One grid at a time, in step order; ctypes releases the GIL inside the library call."""

    def __init__(self, fs, n, d, stream):
        super().__init__(daemon=True)
        self.fs, self.n, self.d, self.stream = fs, n, d, stream
        self.cv = threading.Condition()
        self.job, self.done, self.quit, self.busy_s = None, 0, False, 0.0

    def run(self):
        while True:
            with self.cv:
                self.cv.wait_for(lambda: self.job is not None or self.quit)
                if self.job is None:
                    return
                i, g = self.job
            t0 = time.perf_counter()
            path = os.path.join(self.d, f"mygrids{i}.vdb")
            w = self.fs.VdbStream(path, self.n, 1)
            hs = (C.c_void_p * 2)(w._h.value, self.stream._h.value)
            self.fs.check(self.fs.lib.fluid_vdb_append_leaves(hs, 2, C.byref(g)))
            w.close()
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


def run(fs, n, ppc, mode, steps, warmup, late):
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.reference_scatter() if (n, ppc) == (121, 10) else fs.water_cube_drop(n, ppc, seed=0))
    for _ in range(late + warmup):
        sim.step()
    out = {"mode": mode}
    with tempfile.TemporaryDirectory() as d:
        stream = fs.VdbStream(os.path.join(d, "mygrids.vdb"), n, steps) if mode != "none" else None
        wr = None
        if mode == "leaves":
            wr = Writer(fs, n, d, stream)
            wr.start()
        listed, to_host = [], []
        t0 = time.perf_counter()
        for i in range(steps):
            sim.step()
            if mode == "dense":
                f = sim.field(fs.FIELD.OUTPUT)
                path = os.path.join(d, f"mygrids{i}.vdb")
                fs.write_vdb(path, f)
                stream.append(f)
                os.unlink(path)
            elif mode == "leaves":
                wr.wait_done(i - 1)
                sim.output_snapshot()
                st = sim.output_stats()
                listed.append(st["leaves_listed"]); to_host.append(st["bytes_to_host"])
                out["leaves_in_grid"] = st["leaves_in_grid"]
                if i > 0:
                    g = fs.LeafGridC()
                    fs.check(fs.lib.fluid_output_wait(sim._h, C.byref(g)))
                    wr.submit(i - 1, g)
        if mode == "leaves":
            g = fs.LeafGridC()
            fs.check(fs.lib.fluid_output_wait(sim._h, C.byref(g)))
            wr.submit(steps - 1, g)
            wr.wait_done(steps)
        out["ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
        if wr:
            wr.stop()
            out["writer_busy_ms_per_step"] = wr.busy_s / steps * 1e3
            out["leaves_listed_mean"] = sum(listed) / steps
            out["leaves_listed_max"] = max(listed)
            out["bytes_to_host_mean"] = sum(to_host) / steps
        if stream:
            stream.close()
            out["stream_bytes"] = os.path.getsize(os.path.join(d, "mygrids.vdb"))
    sim.close()
    return out


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("void ", "").replace("fl::", ""))
            if name in NEW_KERNELS:
                a = acc.setdefault(name, [])
                a.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "mean_us": sum(v) / len(v), "min_us": min(v), "max_us": max(v)} for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--late", type=int, default=0)
    ap.add_argument("--only", choices=MODES)
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    res = {"n": a.n, "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "late": a.late, "runs": {m: [] for m in MODES}}
    for k in range(a.runs):
        for m in ([a.only] if a.only else MODES):
            r = run(fs, a.n, a.ppc, m, a.steps, a.warmup, a.late)
            res["runs"][m].append(r)
            extra = ""
            if m == "leaves":
                extra = (f"  leaves {r['leaves_listed_mean']:.0f} / {r['leaves_in_grid']} (max {r['leaves_listed_max']})  "
                         f"to host {r['bytes_to_host_mean'] / 1e6:.2f} MB/step  writer busy {r['writer_busy_ms_per_step']:.2f} ms/step")
            print(f"n={a.n} late={a.late} run {k} {m:6s} {r['ms_per_step']:9.3f} ms/step{extra}", flush=True)
    ms = {m: [r["ms_per_step"] for r in v] for m, v in res["runs"].items() if v}
    if all(m in ms for m in MODES):
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        spread = max(ms["dense"]) - min(ms["dense"])
        res["summary"] = {"median_ms": med, "dense_spread_ms": spread, "dense_over_leaves": med["dense"] / med["leaves"],
                          "leaves_minus_none_ms": med["leaves"] - med["none"]}
        print(f"median ms/step: none {med['none']:.3f}  dense {med['dense']:.3f} (spread {spread:.3f})  leaves {med['leaves']:.3f}  "
              f"dense/leaves {med['dense'] / med['leaves']:.1f}x  leaves - none {med['leaves'] - med['none']:+.3f}", flush=True)
    if a.prof:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--n", str(a.n), "--ppc", str(a.ppc), "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--late", str(a.late), "--runs", "1", "--only", "leaves"]
            subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
            res["kernels"] = kernel_times(d)
        for k, v in sorted(res["kernels"].items()):
            print(f"{k:12s} {v['launches']:5d} launches  mean {v['mean_us']:8.2f} us  min {v['min_us']:8.2f}  max {v['max_us']:8.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
