#!/usr/bin/env python3
"""What growing the band of the tracked liquid surface costs per snapshot:
python tools/grow_cost.py [--n 256] [--ppc 8] [--steps 20] [--warmup 5] [--runs 3] [--radius 1.5] [--half-width 2.5]
                          [--offset -1.0] [--parent DIR] [--prof]

Wall ms per step of the same steps in these forms (the scene of tools/track_cost.py: bench.py's drop), each in a fresh handle,
alternated `--runs` times in one call:
  none       no output
  track      fluid_sdf_snapshot_filtered with (width, iterations, offset) = (1, 4, --offset) after the step and fluid_sdf_set_track
             (3, 1), fluid_sdf_wait one step later: growing off
  grow       the same with fluid_sdf_set_track_grow(1): one dilation launch per track, and the range dilated by T cells more
  parent     with --parent DIR, a built checkout of the commit before the growing: its `track` form, one child process per run
             (two builds of the library do not share a process)
Per form the leaves listed by the last step's snapshot.  The addends `form - none` come from the same run of this script.
Then, in a child process of its own with FLUID_SDF_GROW_STATS=1 (which adds two host waits per snapshot and is therefore not timed):
the leaves in range, the leaves the search flagged, the leaves flagged after the last track and the bytes of per-leaf scratch, for
`track` and for `grow`.
--prof: the `grow` form again under `rocprofv3 --kernel-trace --stats` (a child process, a run of its own): times of k_sdf_grow,
k_sdf_track, k_sdf_relist, k_sdf_box, k_sdf_offset, of the k_sdf_* kernels of the front half and of the scan."""
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

TRACK = (3, 1, 0)
FORMS = ["none", "track", "grow", "parent"]


def run(fs, a, form):
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    for _ in range(a.warmup):
        sim.step()
    out = {"form": form}
    prm = fs.SdfParams(a.radius, a.half_width)
    filt = fs.SdfFilter(1, 4, a.offset)
    if form in ("track", "grow"):
        fs.check(fs.lib.fluid_sdf_set_track(sim._h, C.byref(fs.SdfTrack(*TRACK))))
    if form == "grow":
        fs.check(fs.lib.fluid_sdf_set_track_grow(sim._h, 1))
    g = fs.SdfGridC()
    snap_s = 0.0
    t0 = time.perf_counter()
    for i in range(a.steps):
        sim.step()
        if form == "none":
            continue
        t1 = time.perf_counter()
        fs.check(fs.lib.fluid_sdf_snapshot_filtered(sim._h, C.byref(prm), C.byref(filt)))
        snap_s += time.perf_counter() - t1
        if i > 0:
            fs.check(fs.lib.fluid_sdf_wait(sim._h, C.byref(g)))
    if form != "none":
        fs.check(fs.lib.fluid_sdf_wait(sim._h, C.byref(g)))
        out["leaves_listed_last"] = g.n_leaves
        out["snapshot_call_ms"] = snap_s / a.steps * 1e3
    out["ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
    out["particles"] = sim.num_particles
    sim.close()
    return out


def child_args(a, form):
    return ["--n", str(a.n), "--ppc", str(a.ppc), "--steps", str(a.steps), "--warmup", str(a.warmup), "--radius", str(a.radius),
            "--half-width", str(a.half_width), "--offset", str(a.offset), "--runs", "1", "--only", form]


def run_parent(a):
    """The `track` form of the tree at a.parent, in a process of its own; its last line is the JSON."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", os.path.abspath(a.parent)] + child_args(a, "track"),
                       check=True, timeout=900, capture_output=True, text=True)
    out = json.loads(r.stdout.strip().splitlines()[-1])["runs"]["track"][0]
    out["form"] = "parent"
    return out


def leaf_stats(a, form):
    """The last `sdf grow:` line of a child run of `form` with FLUID_SDF_GROW_STATS=1."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + child_args(a, form), check=True, timeout=900, capture_output=True, text=True,
                       env=dict(os.environ, FLUID_SDF_GROW_STATS="1"))
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("sdf grow:")]
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", lines[-1])} if lines else {}


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"[<(].*", "", r["Kernel_Name"].replace("void ", "").replace("fl::", ""))
            if name.startswith(("k_sdf_", "k_scan_")):
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
    ap.add_argument("--offset", type=float, default=-1.0)
    ap.add_argument("--only", choices=FORMS[:3])
    ap.add_argument("--parent", help="a built checkout of the commit before the growing")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is loaded (default: this one)")
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    import __graft_entry__ as entry
    fs = entry.load_package()
    forms = [a.only] if a.only else [f for f in FORMS if f != "parent" or a.parent]
    res = {"n": a.n, "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "radius": a.radius, "half_width": a.half_width,
           "filter": (1, 4, a.offset), "track": TRACK, "runs": {f: [] for f in forms}}
    for k in range(a.runs):
        for f in forms:
            r = run_parent(a) if f == "parent" else run(fs, a, f)
            res["runs"][f].append(r)
            extra = "" if f == "none" else f"  leaves listed {r['leaves_listed_last']}  snapshot call {r['snapshot_call_ms']:.2f} ms"
            print(f"n={a.n} run {k} {f:6s} {r['ms_per_step']:9.3f} ms/step{extra}", flush=True)
    if not a.only:
        ms = {f: [r["ms_per_step"] for r in v] for f, v in res["runs"].items()}
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        res["summary"] = {"median_ms": med, "none_spread_ms": max(ms["none"]) - min(ms["none"]),
                          "minus_none_ms": {f: med[f] - med["none"] for f in forms if f != "none"},
                          "grow_minus_track_ms": med["grow"] - med["track"]}
        print("median ms/step: " + "  ".join(f"{f} {med[f]:.3f}" for f in forms) + f"  (none spread {res['summary']['none_spread_ms']:.3f})  " +
              f"grow - track {med['grow'] - med['track']:+.3f}", flush=True)
        res["leaves"] = {f: leaf_stats(a, f) for f in ("track", "grow")}
        for f, v in res["leaves"].items():
            print(f"{f:6s} " + "  ".join(f"{k} {x}" for k, x in v.items()), flush=True)
    if a.prof:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__)] + \
                child_args(a, "grow")
            subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
            res["kernels"] = kernel_times(d)
        for k, v in sorted(res["kernels"].items()):
            print(f"{k:18s} {v['launches']:5d} launches  mean {v['mean_us']:9.2f} us  min {v['min_us']:9.2f}  max {v['max_us']:9.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
