#!/usr/bin/env python3
"""What the velocity trails' rank record of a decomposed run costs beside the spheres':
python tools/trail_cost_blocks.py [--n 256] [--ppc 8] [--at 0 200 445] [--reps 7] [--radius 1] [--half-width 2]

One 2 x 2 x 2 block run of water_cube_drop (threads of this process over the in-process transport, ALL EIGHT BLOCKS ON ONE GPU).  After
each of the steps named by --at (0: after the upload) the run stops, and the ranks, ONE AT A TIME so that no rank's figure holds
another's work, take in turns `--reps` times after one untimed round that sizes the buffers and loads the code
  spheres   fluid_dist_sdf_snapshot + fluid_dist_sdf_wait: the parent's rank record
  trails    fluid_dist_sdf_snapshot_trails + fluid_dist_sdf_wait with shutter = the dt_out of the step just taken (at step 0: the
            first step's dt of 0.1), delta 1, radius_min R / 2, at most 16 instances: the loop of
            `FLUID_BLOCKS=2x2x2 FLUID_BLOCKS_SURFACE=R,W FLUID_BLOCKS_SURFACE_TRAILS=dt ./run.sh fluid`
and the wall time of each pair is a host clock from the call to the end of its wait (the call reads the box and the counts back,
the wait ends with the copy: both end in device synchronises).  Per rank: median (min, max) ms of both, instances per live
particle, leaves listed and bytes to the host.  Then the host merge (fluid_sdf_grids_merge, its count and its fill) of the eight
lists of either kind, `--reps` times on one thread.  Nothing is asserted or thresholded; eight blocks on one GPU say nothing about
scaling over real peers.  The result goes to profiles/trail/blocks_<n>.json."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (2, 2, 2)


def spread(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]}


def merge_ms(fs, parts, size, reps):
    """ms of the count and the fill of fluid_sdf_grids_merge over the ranks' lists, and the merged leaf count."""
    merge, ms, k = fs.lib.fluid_sdf_grids_merge, [], 0
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        k = merge(parts, size, 0, None, None, None)
        assert k >= 0
        org, val, act = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.empty((k, 8), np.uint64)
        assert k == 0 or merge(parts, size, k, *[x.ctypes.data_as(C.c_void_p) for x in (org, val, act)]) == k
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms[1:]), int(k)


def run(fs, fd, n, ppc, at, reps, R, w):
    size = DIMS[0] * DIMS[1] * DIMS[2]
    pos = fs.water_cube_drop(n, ppc, seed=0)
    cuts = fd.partition_blocks(n, pos, DIMS)
    grp = fd.LocalGroup(size)
    sims = [None] * size
    prm = fs.SdfParams(R, w)
    parts = {m: (fs.SdfGridC * size)() for m in ("spheres", "trails")}
    bar = threading.Barrier(size)
    points = []

    def work(r):
        try:
            return block(r)
        except BaseException:
            bar.abort()                         # nobody is left waiting at the barrier
            raise

    def measure(sim, r, step, dt):
        trl = fs.SdfTrails(dt, 1.0, R / 2, 16, 0)
        forms = {"spheres": lambda: fs.lib.fluid_dist_sdf_snapshot(sim._h, C.byref(prm)),
                 "trails": lambda: fs.lib.fluid_dist_sdf_snapshot_trails(sim._h, C.byref(prm), C.byref(trl))}
        ms = {m: [] for m in forms}
        row = {"rank": r, "live": sim.num_live()}
        for k in range(reps + 1):               # (round 0 sizes the buffers and loads the code: not timed)
            for m, snap in forms.items():
                t0 = time.perf_counter()
                fs.check(snap())
                fs.check(fs.lib.fluid_dist_sdf_wait(sim._h, C.byref(parts[m][r])))
                if k:
                    ms[m].append((time.perf_counter() - t0) * 1e3)
                row[m + "_leaves"] = parts[m][r].n_leaves
                row[m + "_bytes_to_host"] = sim.sdf_stats()["bytes_to_host"]
        ts = sim.sdf_dist_trails_stats()
        row.update(spheres_ms=spread(ms["spheres"]), trails_ms=spread(ms["trails"]), instances=ts["instances"],
                   instances_per_live_particle=ts["instances"] / max(1, ts["particles"]))
        assert ts["particles"] == row["live"]
        return row

    def block(r):
        sim = fd.DistFluidSim(n, DIMS, cuts, grp.comms[r])
        sims[r] = sim
        sim.upload_global(pos)
        dt, step = 0.1, 0
        for stop in at:
            while step < stop:
                dt = sim.step()["dt_out"]
                step += 1
            for turn in range(size):            # one rank at a time
                bar.wait()
                if turn == r:
                    rank_rows[r].append(measure(sim, r, step, dt))
            if r == 0:
                points.append({"step": step, "dt": dt})
            bar.wait()
            if r == 0:                          # every rank's last two lists are in `parts`, and stay until its next snapshot
                p = points[-1]
                for m in ("spheres", "trails"):
                    p[m + "_merge_ms"], p[m + "_merged_leaves"] = merge_ms(fs, parts[m], size, reps)
            bar.wait()
        return 0

    rank_rows = [[] for _ in range(size)]
    try:
        grp.run(work)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    for i, p in enumerate(points):
        p["ranks"] = [rank_rows[r][i] for r in range(size)]
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--at", type=int, nargs="+", default=[0, 200, 445])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--half-width", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trail"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    fd = fs.load_dist()
    os.makedirs(a.out, exist_ok=True)
    points = run(fs, fd, a.n, a.ppc, sorted(a.at), a.reps, a.radius, a.half_width)
    res = {"n": a.n, "dims": list(DIMS), "ppc": a.ppc, "reps": a.reps, "radius": a.radius, "half_width": a.half_width,
           "trails": {"shutter": "dt_out", "delta": 1.0, "radius_min": a.radius / 2, "max_instances": 16}, "points": points}
    for p in points:
        print(f"step {p['step']} dt {p['dt']:.6g}: merge ms spheres {p['spheres_merge_ms']['median']:.3f} ({p['spheres_merged_leaves']} leaves) "
              f"trails {p['trails_merge_ms']['median']:.3f} ({p['trails_merged_leaves']} leaves)")
        for q in p["ranks"]:
            s, t = q["spheres_ms"], q["trails_ms"]
            print(f"  rank {q['rank']} live {q['live']:8d}  spheres {s['median']:7.3f} ({s['min']:.3f} .. {s['max']:.3f}) ms  trails {t['median']:7.3f} "
                  f"({t['min']:.3f} .. {t['max']:.3f}) ms  x{t['median'] / s['median']:.2f}  instances/particle {q['instances_per_live_particle']:.3f}  "
                  f"leaves {q['spheres_leaves']} / {q['trails_leaves']}  bytes {q['spheres_bytes_to_host']} / {q['trails_bytes_to_host']}", flush=True)
    with open(os.path.join(a.out, f"blocks_{a.n}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
