#!/usr/bin/env python3
"""What the velocity trails cost beside the spheres': python tools/trail_cost.py [--n 256] [--ppc 8] [--at 0 200 445] [--reps 7]
                                                        [--radius 1.0] [--half-width 2.0] [--delta 1.0] [--max-instances 16] [--prof]

One handle, the drop scene; on the state after each of the `--at` step counts (0: right after the upload, where nothing moves),
the wall time of one level-set snapshot from the call to the end of its wait (both end in a device synchronise), in four forms
that take turns `--reps` times after one round that sizes the buffers:
  spheres                 fluid_sdf_snapshot of the particles, the setting cleared
  trails Rm=R/2           the same call under fluid_sdf_set_trails(shutter = the last step's dt, delta, R / 2)
  trails Rm=R             and with a constant radius: k_sdf_search_rad over N items that all have radius R
  spheres of instances    the YARDSTICK: a second handle whose particles are the N host-expanded instance positions of the form
                          before (fluid_particles_trails), the setting cleared: k_sdf_search over the same N items, the same level set
The last two differ in the expansion (two passes and a scan), in the scatter (the radius rides along) and in the search; bbox or
count pass, bin, scan of the flags, pack and copy are alike.  Instances per particle are printed beside the times.
--prof: each form again under `rocprofv3 --kernel-trace --stats` (a child process per form, a run of its own): launches and times
of k_trail_count, k_trail_expand, k_trail_scatter, k_sdf_bbox, k_sdf_count, k_sdf_scatter, k_sdf_search_rad, k_sdf_search and
k_sdf_pack at the last of the `--at` states (the scans carry the same names as the steps' and are left out)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("spheres", "trails Rm=R/2", "trails Rm=R", "spheres of instances")


class Scene:
    """The handle at one state, and the second handle that holds the instances of `trails Rm=R` as particles."""

    def __init__(self, fs, a, sim, dt):
        self.fs, self.a, self.sim, self.dt = fs, a, sim, dt
        pos, vel = sim.download_particles()
        P, _ = fs.particles_trails(pos, vel, a.radius, a.half_width, dt, a.delta, a.radius, a.max_instances)
        self.items = len(P)
        self.other = fs.FluidSim(n=a.n)
        self.other.upload_particles(P)

    def one(self, form):
        a, sim = self.a, self.sim
        if form == "spheres of instances":
            sim = self.other
        elif form == "spheres":
            sim.sdf_set_trails(None)
        else:
            sim.sdf_set_trails(self.dt, a.delta, a.radius / 2 if form == "trails Rm=R/2" else a.radius, a.max_instances)
        t0 = time.perf_counter()
        sim.sdf_snapshot(a.radius, a.half_width)
        g = sim.sdf_wait()
        ms = (time.perf_counter() - t0) * 1e3
        inst = sim.sdf_trails_stats()["instances"] if form.startswith("trails") else sim.num_particles
        return ms, g.n_leaves, inst

    def close(self):
        self.sim.sdf_set_trails(None)
        self.other.close()


def measure(sc, forms, reps, state, res):
    for f in forms:                                       # sizes the buffers, loads the code objects
        sc.one(f)
    ms, last = {f: [] for f in forms}, {}
    for _ in range(reps):
        for f in forms:
            t, k, inst = sc.one(f)
            ms[f].append(t)
            last[f] = (k, inst)
    npart = sc.sim.num_particles
    res[state] = {"particles": npart, "dt": sc.dt}
    for f in forms:
        v = sorted(ms[f])
        res[state][f] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "leaves_listed": last[f][0], "items": last[f][1]}
        print(f"n={sc.a.n} {state:10s} {f:22s} {v[len(v) // 2]:9.3f} ms  ({v[0]:.3f} ... {v[-1]:.3f})  leaves {last[f][0]}  items {last[f][1]}"
              f"  ({last[f][1] / npart:.3f} per particle)", flush=True)


def kernel_times(d):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("void ", "").replace("fl::", "").split("(")[0]
            if name.startswith(("k_trail_", "k_sdf_")):       # (the scans are the steps' sort's as well: left out)
                acc.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "mean_us": sum(v) / len(v), "min_us": min(v), "max_us": max(v)} for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--at", type=int, nargs="+", default=[0, 200, 445])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--half-width", type=float, default=2.0)
    ap.add_argument("--delta", type=float, default=1.0)
    ap.add_argument("--max-instances", type=int, default=16)
    ap.add_argument("--only", choices=FORMS)
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    forms = [a.only] if a.only else list(FORMS)
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    res = {k: getattr(a, k) for k in ("n", "ppc", "at", "reps", "radius", "half_width", "delta", "max_instances")}
    done, dt = 0, sim.stats()["dt_out"]
    for at in sorted(a.at):
        for _ in range(at - done):
            dt = sim.step()["dt_out"]
        done = at
        sc = Scene(fs, a, sim, dt)
        measure(sc, forms, a.reps, f"step {at}", res)
        sc.close()
    sim.close()
    res["kernels"] = {}
    if a.prof:
        for form in FORMS:
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                       "--n", str(a.n), "--ppc", str(a.ppc), "--at", str(max(a.at)), "--reps", str(a.reps), "--radius", str(a.radius),
                       "--half-width", str(a.half_width), "--delta", str(a.delta), "--max-instances", str(a.max_instances), "--only", form]
                subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
                res["kernels"][form] = kernel_times(d)
            for k, v in sorted(res["kernels"][form].items()):
                print(f"{form:22s} {k:40s} {v['launches']:5d} launches  mean {v['mean_us']:10.2f} us  min {v['min_us']:10.2f}  max {v['max_us']:10.2f}",
                      flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
