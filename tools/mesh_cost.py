#!/usr/bin/env python3
"""What the liquid surface costs per step as a file of leaves and as a mesh:
python tools/mesh_cost.py [--n 256] [--ppc 8] [--steps 20] [--warmup 5] [--runs 3] [--late 0] [--radius 1.5] [--half-width 2.5] [--prof]

Wall ms per step of the same steps in three forms (the scenes of tools/sdf_cost.py), each in a fresh handle, `--runs` times:
  none     no output
  surface  the level set of the particles: fluid_sdf_snapshot after the step, fluid_sdf_wait one step later, a writer thread
           writes surface<i>.vdb with fluid_write_vdb_sdf (tools/sdf_cost.py's `surface`)
  mesh     its surface nets: fluid_mesh_snapshot after the step, fluid_mesh_wait one step later, a writer thread writes
           mesh<i>.ply with fluid_write_ply_mesh
The addends `surface - none` and `mesh - none`, and the writer thread's busy time per file, come from the same run of this script.
--late K: K steps without output first.  --prof: the `mesh` form again under `rocprofv3 --kernel-trace --stats` (a child process,
a run of its own): times of the k_mesh_* kernels, of the k_sdf_* kernels of the shared front half and of the scan."""
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

MODES = ("none", "surface", "mesh")


class Writer(threading.Thread):
    """One file at a time, in step order; ctypes releases the GIL inside the library call."""

    def __init__(self, fs, d, mode, voxel):
        super().__init__(daemon=True)
        self.fs, self.d, self.mode, self.voxel = fs, d, mode, voxel
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
            if self.mode == "surface":
                path = os.path.join(self.d, f"surface{i}.vdb")
                fs.check(fs.lib.fluid_write_vdb_sdf(path.encode(), C.byref(g), 3))
            else:
                path = os.path.join(self.d, f"mesh{i}.ply")
                fs.check(fs.lib.fluid_write_ply_mesh(path.encode(), C.byref(g), self.voxel))
            self.busy_s += time.perf_counter() - t0
            self.file_bytes += os.path.getsize(path)
            os.unlink(path)
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
        wr = None
        if mode != "none":
            wr = Writer(fs, d, mode, 1.0)
            wr.start()

        def wait():
            if mode == "surface":
                g = fs.SdfGridC()
                fs.check(fs.lib.fluid_sdf_wait(sim._h, C.byref(g)))
            else:
                g = fs.MeshC()
                fs.check(fs.lib.fluid_mesh_wait(sim._h, C.byref(g)))
            return g
        to_host, snap_s = [], 0.0
        t0 = time.perf_counter()
        for i in range(steps):
            sim.step()
            if mode == "none":
                continue
            wr.wait_done(i - 1)
            t1 = time.perf_counter()
            if mode == "surface":
                fs.check(fs.lib.fluid_sdf_snapshot(sim._h, C.byref(prm)))
                st = sim.sdf_stats()
                out["leaves_listed_last"] = st["leaves_listed"]
            else:
                fs.check(fs.lib.fluid_mesh_snapshot(sim._h, C.byref(prm)))
                st = sim.mesh_stats()
                out["vertices_last"], out["quads_last"] = st["vertices"], st["quads"]
            snap_s += time.perf_counter() - t1
            to_host.append(st["bytes_to_host"])
            if i > 0:
                wr.submit(i - 1, wait())
        if wr:
            wr.submit(steps - 1, wait())
            wr.wait_done(steps)
        out["ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
        if wr:
            wr.stop()
            out["writer_busy_ms_per_file"] = wr.busy_s / steps * 1e3
            out["snapshot_call_ms"] = snap_s / steps * 1e3
            out["bytes_to_host_mean"] = sum(to_host) / steps
            out["file_bytes_mean"] = wr.file_bytes / steps
    out["particles"] = sim.num_particles
    sim.close()
    return out


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"[<(].*", "", r["Kernel_Name"].replace("void ", "").replace("fl::", ""))
            if name.startswith(("k_mesh_", "k_sdf_", "k_scan_")):
                acc.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "mean_us": sum(v) / len(v), "min_us": min(v), "max_us": max(v)} for k, v in acc.items()}


def child_args(a):
    return [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--ppc", str(a.ppc), "--steps", str(a.steps), "--warmup", str(a.warmup),
            "--late", str(a.late), "--radius", str(a.radius), "--half-width", str(a.half_width), "--runs", "1", "--only", "mesh"]


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
                what = f"leaves {r['leaves_listed_last']}" if m == "surface" else f"vertices {r['vertices_last']} quads {r['quads_last']}"
                extra = (f"  {what}  to host {r['bytes_to_host_mean'] / 1e6:.2f} MB/step  file {r['file_bytes_mean'] / 1e6:.2f} MB  "
                         f"snapshot call {r['snapshot_call_ms']:.2f} ms  writer busy {r['writer_busy_ms_per_file']:.2f} ms/file")
            print(f"n={a.n} late={a.late} run {k} {m:7s} {r['ms_per_step']:9.3f} ms/step{extra}", flush=True)
    ms = {m: [r["ms_per_step"] for r in v] for m, v in res["runs"].items() if v}
    if all(m in ms for m in MODES):
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        busy = {m: sorted(r["writer_busy_ms_per_file"] for r in res["runs"][m])[len(ms[m]) // 2] for m in ("surface", "mesh")}
        res["summary"] = {"median_ms": med, "none_spread_ms": max(ms["none"]) - min(ms["none"]), "surface_minus_none_ms": med["surface"] - med["none"],
                          "mesh_minus_none_ms": med["mesh"] - med["none"], "writer_busy_ms_per_file": busy}
        print(f"median ms/step: none {med['none']:.3f} (spread {res['summary']['none_spread_ms']:.3f})  surface {med['surface']:.3f}  mesh {med['mesh']:.3f}  "
              f"surface - none {med['surface'] - med['none']:+.3f}  mesh - none {med['mesh'] - med['none']:+.3f}  "
              f"writer busy per file: .vdb {busy['surface']:.2f} ms  .ply {busy['mesh']:.2f} ms", flush=True)
    if a.prof:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + child_args(a)
            subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
            res["kernels"] = kernel_times(d)
        for k, v in sorted(res["kernels"].items()):
            print(f"{k:18s} {v['launches']:5d} launches  mean {v['mean_us']:9.2f} us  min {v['min_us']:9.2f}  max {v['max_us']:9.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
