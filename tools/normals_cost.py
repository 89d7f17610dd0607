#!/usr/bin/env python3
"""What the mesh's normals and triangles add to a snapshot per step:
python tools/normals_cost.py [--n 256] [--ppc 8] [--steps 20] [--warmup 5] [--runs 3] [--radius 1.5] [--half-width 2.5] [--prof FORM ...]

Wall ms per step of the same steps in four forms (the scene of tools/mesh_cost.py), each in a fresh handle, alternated `--runs`
times in one call:
  none               no output
  mesh               fluid_mesh_snapshot after the step, fluid_mesh_wait one step later (no file is written)
  mesh_normals       fluid_mesh_snapshot_ex(FLUID_MESH_NORMALS) / fluid_mesh_wait_ex: a unit normal per vertex
  mesh_normals_tris  fluid_mesh_snapshot_ex(FLUID_MESH_NORMALS | FLUID_MESH_TRIANGLES): and two triangles per quad (k_mesh_tris)
Per form what the last snapshot sent to the host.  The addends `form - none`, `mesh_normals - mesh` and `mesh_normals_tris - mesh`
come from the same run of this script; the spread of `none` over the runs is printed beside them.  To read `mesh` against the commit
before the options existed, run that commit's tools/attr_cost.py (its `mesh` form is this one) in the same session.
--prof FORM (may be given more than once): that form again under `rocprofv3 --kernel-trace --stats` (a child process, a run of its
own, no counters): times of the k_sdf_*, k_mesh_* and scan kernels, the template arguments kept (k_mesh_emit<false, false> is the
plain emit, <false, true> the one that writes normals).  Nothing is asserted or thresholded."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("none", "mesh", "mesh_normals", "mesh_normals_tris")


def run(fs, a, form):
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    for _ in range(a.warmup):
        sim.step()
    out = {"form": form}
    prm = fs.SdfParams(a.radius, a.half_width)
    m, ex = fs.MeshC(), fs.MeshExC()
    what = {"mesh_normals": fs.MESH.NORMALS, "mesh_normals_tris": fs.MESH.NORMALS | fs.MESH.TRIANGLES}.get(form)
    snap = {"mesh": lambda: fs.lib.fluid_mesh_snapshot(sim._h, C.byref(prm)),
            "mesh_normals": lambda: fs.lib.fluid_mesh_snapshot_ex(sim._h, C.byref(prm), None, what),
            "mesh_normals_tris": lambda: fs.lib.fluid_mesh_snapshot_ex(sim._h, C.byref(prm), None, what)}.get(form)
    wait = {"mesh": lambda: fs.lib.fluid_mesh_wait(sim._h, C.byref(m)),
            "mesh_normals": lambda: fs.lib.fluid_mesh_wait_ex(sim._h, C.byref(m), C.byref(ex)),
            "mesh_normals_tris": lambda: fs.lib.fluid_mesh_wait_ex(sim._h, C.byref(m), C.byref(ex))}.get(form)
    snap_s = 0.0
    t0 = time.perf_counter()
    for i in range(a.steps):
        sim.step()
        if snap is None:
            continue
        t1 = time.perf_counter()
        fs.check(snap())
        snap_s += time.perf_counter() - t1
        if i > 0:
            fs.check(wait())
    if snap is not None:
        fs.check(wait())
        out["snapshot_call_ms"] = snap_s / a.steps * 1e3
        out["last"] = sim.mesh_stats()
    out["ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
    out["particles"] = sim.num_particles
    sim.close()
    return out


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("void ", "").replace("fl::", "").split("(")[0]
            if name.startswith(("k_mesh_", "k_sdf_", "k_scan_")):
                acc.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "mean_us": sum(v) / len(v), "min_us": min(v), "max_us": max(v)} for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--half-width", type=float, default=2.5)
    ap.add_argument("--only", choices=FORMS)
    ap.add_argument("--prof", action="append", choices=FORMS[1:], default=[])
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    forms = [a.only] if a.only else list(FORMS)
    res = {"n": a.n, "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "radius": a.radius, "half_width": a.half_width, "runs": {f: [] for f in forms}}
    for k in range(a.runs):
        for f in forms:
            r = run(fs, a, f)
            res["runs"][f].append(r)
            extra = "" if f == "none" else f"  {r['last']}  snapshot call {r['snapshot_call_ms']:.2f} ms"
            print(f"n={a.n} run {k} {f:18s} {r['ms_per_step']:9.3f} ms/step{extra}", flush=True)
    if not a.only:
        ms = {f: [r["ms_per_step"] for r in v] for f, v in res["runs"].items()}
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        res["summary"] = {"median_ms": med, "none_spread_ms": max(ms["none"]) - min(ms["none"]),
                          "minus_none_ms": {f: med[f] - med["none"] for f in forms if f != "none"},
                          "minus_mesh_ms": {f: med[f] - med["mesh"] for f in forms[2:]}}
        print("median ms/step: " + "  ".join(f"{f} {med[f]:.3f}" for f in forms) + f"  (none spread {res['summary']['none_spread_ms']:.3f})  " +
              "  ".join(f"{f} - mesh {med[f] - med['mesh']:+.3f}" for f in forms[2:]), flush=True)
    res["kernels"] = {}
    for form in a.prof:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--n", str(a.n), "--ppc", str(a.ppc), "--steps", str(a.steps), "--warmup", str(a.warmup), "--radius", str(a.radius),
                   "--half-width", str(a.half_width), "--runs", "1", "--only", form]
            subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
            res["kernels"][form] = kernel_times(d)
        for k, v in sorted(res["kernels"][form].items()):
            print(f"{form:18s} {k:34s} {v['launches']:5d} launches  mean {v['mean_us']:9.2f} us  min {v['min_us']:9.2f}  max {v['max_us']:9.2f}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
