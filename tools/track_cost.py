#!/usr/bin/env python3
"""What renormalising the smoothed liquid surface adds to a mesh per step:
python tools/track_cost.py [--n 256] [--ppc 8] [--steps 20] [--warmup 5] [--runs 3] [--radius 1.5] [--half-width 2.5]
                           [--scheme first|hjweno5|both] [--parent DIR] [--prof]

Wall ms per step of the same steps in these forms (the scene of tools/smooth_cost.py), each in a fresh handle, alternated `--runs`
times in one call:
  none       no output
  smooth     fluid_mesh_snapshot_filtered with (width, iterations, offset) = (1, 4, 0) after the step, fluid_mesh_wait one step
             later: 12 box passes
  track      the same with fluid_sdf_set_track (3, 1): 12 box passes, 12 normalisation passes (the trim on every third), 1 relist
  weno       with --scheme both: `track` with the scheme FLUID_SDF_TRACK_HJWENO5 beside it, alternated with the others; --scheme hjweno5
             makes `track` itself run that scheme (the default, first, is the first-order scheme)
  parent     with --parent DIR, a built checkout of the commit before the tracking: its `smooth` form, one child process per run
             (two builds of the library do not share a process)
Per form the vertices and quads of the last step's mesh.  The addends `form - none` come from the same run of this script.
--prof: the `track` form again under `rocprofv3 --kernel-trace --stats` (a child process, a run of its own): times of k_sdf_track,
k_sdf_relist, k_sdf_box, of the k_mesh_* kernels, of the k_sdf_* kernels of the front half and of the scan; with --scheme hjweno5 or
both the same for k_sdf_track_weno (both: one profiled run per scheme)."""
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILTER = (1, 4, 0.0)
TRACK = (3, 1, 0)
SCHEMES = {"first": 0, "hjweno5": 4}
FORMS = ["none", "smooth", "track", "weno", "parent"]


def run(fs, a, form):
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    for _ in range(a.warmup):
        sim.step()
    out = {"form": form}
    prm = fs.SdfParams(a.radius, a.half_width)
    filt = fs.SdfFilter(*FILTER)
    if form in ("track", "weno"):
        scheme = SCHEMES["hjweno5"] if form == "weno" else SCHEMES[a.scheme]
        fs.check(fs.lib.fluid_sdf_set_track(sim._h, C.byref(fs.SdfTrack(TRACK[0], TRACK[1], scheme))))
    m = fs.MeshC()
    snap_s = 0.0
    t0 = time.perf_counter()
    for i in range(a.steps):
        sim.step()
        if form == "none":
            continue
        t1 = time.perf_counter()
        fs.check(fs.lib.fluid_mesh_snapshot_filtered(sim._h, C.byref(prm), C.byref(filt)))
        snap_s += time.perf_counter() - t1
        if i > 0:
            fs.check(fs.lib.fluid_mesh_wait(sim._h, C.byref(m)))
    if form != "none":
        fs.check(fs.lib.fluid_mesh_wait(sim._h, C.byref(m)))
        out["vertices_last"], out["quads_last"] = m.n_vertices, m.n_quads
        out["snapshot_call_ms"] = snap_s / a.steps * 1e3
    out["ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
    out["particles"] = sim.num_particles
    sim.close()
    return out


def child_args(a, form, scheme="first"):
    return ["--scheme", scheme, "--n", str(a.n), "--ppc", str(a.ppc), "--steps", str(a.steps), "--warmup", str(a.warmup), "--radius", str(a.radius),
            "--half-width", str(a.half_width), "--runs", "1", "--only", form]


def run_parent(a):
    """The `smooth` form of the tree at a.parent, in a process of its own; its last line is the JSON."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", os.path.abspath(a.parent)] + child_args(a, "smooth"),
                       check=True, timeout=900, capture_output=True, text=True)
    out = json.loads(r.stdout.strip().splitlines()[-1])["runs"]["smooth"][0]
    out["form"] = "parent"
    return out


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"[<(].*", "", r["Kernel_Name"].replace("void ", "").replace("fl::", ""))
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
    ap.add_argument("--only", choices=FORMS[:3])
    ap.add_argument("--scheme", choices=["first", "hjweno5", "both"], default="first")
    ap.add_argument("--parent", help="a built checkout of the commit before the tracking")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is loaded (default: this one)")
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    import __graft_entry__ as entry
    fs = entry.load_package()
    both = a.scheme == "both"
    if both:
        a.scheme = "first"
    forms = [a.only] if a.only else [f for f in FORMS if (f != "parent" or a.parent) and (f != "weno" or both)]
    res = {"n": a.n, "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "radius": a.radius, "half_width": a.half_width, "filter": FILTER,
           "track": TRACK, "scheme": "both" if both else a.scheme, "runs": {f: [] for f in forms}}
    for k in range(a.runs):
        for f in forms:
            r = run_parent(a) if f == "parent" else run(fs, a, f)
            res["runs"][f].append(r)
            extra = "" if f == "none" else f"  vertices {r['vertices_last']} quads {r['quads_last']}  snapshot call {r['snapshot_call_ms']:.2f} ms"
            print(f"n={a.n} run {k} {f:6s} {r['ms_per_step']:9.3f} ms/step{extra}", flush=True)
    if not a.only:
        ms = {f: [r["ms_per_step"] for r in v] for f, v in res["runs"].items()}
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        res["summary"] = {"median_ms": med, "none_spread_ms": max(ms["none"]) - min(ms["none"]),
                          "minus_none_ms": {f: med[f] - med["none"] for f in forms if f != "none"},
                          "track_minus_smooth_ms": med["track"] - med["smooth"]}
        if both:
            res["summary"]["weno_minus_track_ms"] = med["weno"] - med["track"]
        print("median ms/step: " + "  ".join(f"{f} {med[f]:.3f}" for f in forms) + f"  (none spread {res['summary']['none_spread_ms']:.3f})  " +
              f"track - smooth {med['track'] - med['smooth']:+.3f}", flush=True)
    for scheme in (["first", "hjweno5"] if both else [a.scheme]) if a.prof else []:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__)] + \
                child_args(a, "track", scheme)
            subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
            res.setdefault("kernels", {})[scheme] = kernel_times(d)
        print(f"kernels of the track form, scheme {scheme}:")
        for k, v in sorted(res["kernels"][scheme].items()):
            print(f"{k:18s} {v['launches']:5d} launches  mean {v['mean_us']:9.2f} us  min {v['min_us']:9.2f}  max {v['max_us']:9.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
