#!/usr/bin/env python3
"""What an image of the liquid surface costs:
python tools/render_cost.py [--n 256] [--ppc 8] [--phases 5,195,445] [--window 10] [--reps 9] [--size 1920x1080] [--step 0.5]
                            [--radius 1.5] [--half-width 2.5] [--prof] [--walk none|render|both]

The drop scene is stepped to each phase (at 256^3 and 8 per cell: step 5 is free fall, 195 the splash, 445 the settled pool), and
there, on the state the steps left:
  calls   `--reps` times fluid_render_snapshot (rgb, the camera of fluid_camera_look_at from N * (-0.9, 0.5, -1.2)) + fluid_render_wait
          and as many fluid_mesh_snapshot_ex(what = 6) + fluid_mesh_wait_ex for scale: host clock around a call that ends in the
          wait for the record, the median and the extremes.
  steps   the `--window` steps that follow, with a render snapshot after every step and its wait one step later (walk `render`),
          against the same steps of a second handle that takes none (walk `none`): mean ms per fluid_step call plus what the
          snapshot call adds in between.  Snapshots do not change what the steps compute (tests/test_gpu_render.py), so both walks
          pass through the same states.  That is the price of the feature to a user, not a gate.
--prof: the `calls` part again under `rocprofv3 --kernel-trace --stats` (a child process, a run of its own, no counters): per phase
the median over the reps of the front half's kernels (k_sdf_bbox, _count, _scatter, _search; the scans of a few us are the step's
kernels too and are left out), of k_render_neg + k_render_occ, of k_render_march, and of the mesh's mark and emit.
Nothing is asserted or thresholded."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def walk(fs, a, form, calls):
    """One handle through every phase.  form: none | render (a snapshot per step inside the windows)."""
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    w, h = a.size
    cam = fs.camera_look_at(a.n, (-0.9 * a.n, 0.5 * a.n, -1.2 * a.n), width=w, height=h, step=a.step)
    prm = fs.SdfParams(a.radius, a.half_width)
    img, m, ex = fs.ImageC(), fs.MeshC(), fs.MeshExC()
    out, done = [], 0
    for phase in a.phases:
        while done < phase:
            sim.step()
            done += 1
        rec = {"phase": phase, "form": form, "particles": sim.num_particles}
        if calls:
            tr, tm = [], []
            for k in range(a.reps + 1):   # the first call of each kind sizes the buffers: not counted
                t0 = time.perf_counter()
                fs.check(fs.lib.fluid_render_snapshot(sim._h, C.byref(prm), None, C.byref(cam), None, fs.RENDER.RGB))
                fs.check(fs.lib.fluid_render_wait(sim._h, C.byref(img)))
                t1 = time.perf_counter()
                fs.check(fs.lib.fluid_mesh_snapshot_ex(sim._h, C.byref(prm), None, 6))
                fs.check(fs.lib.fluid_mesh_wait_ex(sim._h, C.byref(m), C.byref(ex)))
                t2 = time.perf_counter()
                if k:
                    tr.append((t1 - t0) * 1e3)
                    tm.append((t2 - t1) * 1e3)
            rec["render_call_ms"], rec["mesh_call_ms"] = med(tr), med(tm)
            rec["hits"], rec["pixels"], rec["render"] = img.n_hit, w * h, sim.render_stats()
            rec["mesh"] = sim.mesh_stats()
            sim.sdf_snapshot(a.radius, a.half_width)
            sim.sdf_wait()
            rec["leaves"] = sim.sdf_stats()
        if a.window > 0 and not a.child:
            step_s = snap_s = 0.0
            for i in range(a.window):
                t0 = time.perf_counter()
                sim.step()
                t1 = time.perf_counter()
                if form == "render":
                    fs.check(fs.lib.fluid_render_snapshot(sim._h, C.byref(prm), None, C.byref(cam), None, fs.RENDER.RGB))
                    if i > 0:
                        fs.check(fs.lib.fluid_render_wait(sim._h, C.byref(img)))
                t2 = time.perf_counter()
                step_s += t1 - t0
                snap_s += t2 - t1
            if form == "render":
                fs.check(fs.lib.fluid_render_wait(sim._h, C.byref(img)))
            done += a.window
            rec["step_ms"], rec["between_steps_ms"] = step_s / a.window * 1e3, snap_s / a.window * 1e3
        out.append(rec)
        print(json.dumps(rec), flush=True)
    sim.close()
    return out


GROUPS = {"front": ("k_sdf_bbox", "k_sdf_count", "k_sdf_scatter", "k_sdf_search"), "occ": ("k_render_neg", "k_render_occ"),
          "march": ("k_render_march",), "mesh": ("k_mesh_mark", "k_mesh_totals", "k_mesh_emit", "k_mesh_tris")}


def kernel_times(d, a):
    """Per phase and group the median over the reps of the group's kernel time per snapshot, us.  The launches of a kernel come in
    the order of the walk: per phase (reps + 1) render snapshots interleaved with as many mesh snapshots, then one surface
    snapshot; the first of each kind per phase (buffers are sized) is left out."""
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("void ", "").replace("fl::", "").split("(")[0].split("<")[0]
            rows.setdefault(name, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    for v in rows.values():
        v.sort()
    out = []
    per = a.reps + 1
    for p, phase in enumerate(a.phases):
        rec = {"phase": phase}
        for g, names in GROUPS.items():
            # front-half kernels run 2 * per + 1 times per phase (render, mesh alternating, then the surface snapshot); the others per
            stride, first = (2 * per + 1, 0) if g == "front" else (per, 0)
            sums = [0.0] * per
            for nm in names:
                v = rows.get(nm, [])
                if len(v) != stride * len(a.phases):
                    rec.setdefault("unexpected_launch_counts", {})[nm] = len(v)
                    continue
                chunk = v[p * stride:(p + 1) * stride]
                for k in range(per):
                    sums[k] += chunk[2 * k][1] if g == "front" else chunk[k][1]   # front: the render snapshot's launch of each pair
            rec[g + "_us"] = med(sums[1:])
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--phases", default="5,195,445")
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--half-width", type=float, default=2.5)
    ap.add_argument("--walk", choices=("none", "render", "both"), default="both")
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.phases = [int(x) for x in a.phases.split(",")]
    a.size = tuple(int(x) for x in a.size.lower().split("x"))
    import __graft_entry__ as entry
    fs = entry.load_package()
    if a.child:
        walk(fs, a, "none", True)
        return
    res = {"args": {k: v for k, v in vars(a).items()}}
    if not a.prof:
        forms = ("none", "render") if a.walk == "both" else (a.walk,)
        res["walks"] = {f: walk(fs, a, f, f == "render") for f in forms}
    else:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child",
                   "--n", str(a.n), "--ppc", str(a.ppc), "--phases", ",".join(map(str, a.phases)), "--reps", str(a.reps), "--size", f"{a.size[0]}x{a.size[1]}",
                   "--step", str(a.step), "--radius", str(a.radius), "--half-width", str(a.half_width)]
            subprocess.run(cmd, check=True, timeout=1100, stdout=subprocess.DEVNULL)
            res["kernels"] = kernel_times(d, a)
        for r in res["kernels"]:
            print(json.dumps(r), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
