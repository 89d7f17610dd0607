#!/usr/bin/env python3
"""What the averaged-position surface of a decomposed run costs beside the spheres':
python tools/avg_cost_blocks.py [--n 128 256] [--ppc 8] [--steps 12] [--warmup 4] [--runs 3] [--radius 1] [--half-width 2] [--influence 3]

Wall ms per step of a 2 x 2 x 2 block run (threads of this process over the in-process transport, all blocks on ONE GPU), in three forms:
  none      no output
  spheres   tools/sdf_cost_blocks.py's `surface`: fluid_dist_sdf_snapshot and fluid_dist_sdf_wait on every block after its step, the
            blocks' lists joined by fluid_sdf_grids_merge on a merger thread while the next step runs (two merge buffers in turn)
  averaged  the same loop with the rank records of the averaged surface: fluid_dist_sdf_snapshot_avg, fluid_dist_sdf_wait_avg and
            fluid_sdf_avg_grids_merge: the loop of `FLUID_BLOCKS=2x2x2 FLUID_BLOCKS_SURFACE=R,W FLUID_BLOCKS_SURFACE_KIND=averaged,H
            ./run.sh fluid` without the file writes
For the two surfaces it reports the bytes the blocks sent to the host in the last step (the known costs of a record: 18 444 bytes per
listed leaf against 2 124, and 32 bytes of scratch per voxel of a block's range for the sums), the sum over the ranks of the listed
leaves against the merged count, and the merger's busy time.  Each form `--runs` times in fresh handles.  The eight blocks share one
GPU here, so the numbers say what the output adds to such a run and nothing about scaling over real peers.
The result goes to profiles/avg/blocks_<n>.json."""
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
MODES = ("none", "spheres", "averaged")


class Merger(threading.Thread):
    """Joins the lists of one step at a time; ctypes releases the GIL inside the library call."""

    def __init__(self, fs, size, averaged):
        super().__init__(daemon=True)
        self.fs, self.size = fs, size
        self.merge = fs.lib.fluid_sdf_avg_grids_merge if averaged else fs.lib.fluid_sdf_grids_merge
        self.cv = threading.Condition()
        self.job, self.done, self.quit, self.busy_s, self.leaves = None, 0, False, 0.0, []
        self.org = [np.empty((0, 3), np.int32), np.empty((0, 3), np.int32)]
        self.val = [np.empty((0, 512), np.float32), np.empty((0, 512), np.float32)]
        self.act = [np.empty((0, 8), np.uint64), np.empty((0, 8), np.uint64)]

    def run(self):
        while True:
            with self.cv:
                self.cv.wait_for(lambda: self.job is not None or self.quit)
                if self.job is None:
                    return
                i, parts = self.job
            t0 = time.perf_counter()
            b = i & 1
            k = self.merge(parts, self.size, 0, None, None, None)
            assert k >= 0
            if len(self.org[b]) < k:
                self.org[b], self.val[b] = np.empty((k + 64, 3), np.int32), np.empty((k + 64, 512), np.float32)
                self.act[b] = np.empty((k + 64, 8), np.uint64)
            o, v, m = (x[b].ctypes.data_as(C.c_void_p) for x in (self.org, self.val, self.act))
            assert k == 0 or self.merge(parts, self.size, k, o, v, m) == k
            self.busy_s += time.perf_counter() - t0
            self.leaves.append(k)
            with self.cv:
                self.job, self.done = None, i + 1
                self.cv.notify_all()

    def submit(self, i, parts):
        with self.cv:
            self.cv.wait_for(lambda: self.job is None)
            self.job = (i, parts)
            self.cv.notify_all()

    def wait_done(self, k):
        with self.cv:
            self.cv.wait_for(lambda: self.done >= k)

    def stop(self):
        with self.cv:
            self.quit = True
            self.cv.notify_all()
        self.join()


def run(fs, fd, n, ppc, mode, steps, warmup, prm, sf):
    size = DIMS[0] * DIMS[1] * DIMS[2]
    pos = fs.water_cube_drop(n, ppc, seed=0)
    cuts = fd.partition_blocks(n, pos, DIMS)
    grp = fd.LocalGroup(size)
    sims = [None] * size
    PartC = fs.SdfAvgPartC if mode == "averaged" else fs.SdfGridC
    parts = [(PartC * size)(), (PartC * size)()]
    listed = [[0] * size for _ in range(steps)]
    bar = threading.Barrier(size)
    mg = Merger(fs, size, mode == "averaged") if mode != "none" else None
    if mg:
        mg.start()
    out = {"mode": mode}
    t = [0.0, 0.0]

    def work(r):
        try:
            return block(r)
        except BaseException:
            bar.abort()                         # nobody is left waiting at the barrier
            raise

    def block(r):
        sim = fd.DistFluidSim(n, DIMS, cuts, grp.comms[r])
        sims[r] = sim
        sim.upload_global(pos)
        for _ in range(warmup):
            sim.step()
        bar.wait()
        if r == 0:
            t[0] = time.perf_counter()
        for i in range(steps):
            sim.step()
            if mode == "averaged":
                fs.check(fs.lib.fluid_dist_sdf_snapshot_avg(sim._h, C.byref(prm), C.byref(sf)))
                fs.check(fs.lib.fluid_dist_sdf_wait_avg(sim._h, C.byref(parts[i & 1][r])))
            elif mode == "spheres":
                fs.check(fs.lib.fluid_dist_sdf_snapshot(sim._h, C.byref(prm)))
                fs.check(fs.lib.fluid_dist_sdf_wait(sim._h, C.byref(parts[i & 1][r])))
            if mode != "none":
                listed[i][r] = parts[i & 1][r].n_leaves
                bar.wait()                      # every block's list of step i is in parts[i & 1]
                if r == 0:
                    mg.submit(i, parts[i & 1])  # (waits for merge i - 1: parts[(i + 1) & 1] is free before step i + 1 ends)
        bar.wait()
        if r == 0:
            if mg:
                mg.wait_done(steps)
            t[1] = time.perf_counter()
        return 0 if mode == "none" else sim.sdf_stats()["bytes_to_host"]

    try:
        res = grp.run(work)
    finally:
        if mg:
            mg.stop()
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    out["ms_per_step"] = (t[1] - t[0]) / steps * 1e3
    if mg:
        out["merged_leaves_mean"] = sum(mg.leaves) / steps
        out["listed_leaves_sum_over_ranks_mean"] = sum(sum(x) for x in listed) / steps
        out["listed_over_merged"] = sum(sum(x) for x in listed) / max(1, sum(mg.leaves))
        out["merge_busy_ms_per_step"] = mg.busy_s / steps * 1e3
        out["bytes_to_host_last_step_all_blocks"] = int(sum(res))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--half-width", type=float, default=2.0)
    ap.add_argument("--influence", type=float, default=3.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avg"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    fd = fs.load_dist()
    os.makedirs(a.out, exist_ok=True)
    prm, sf = fs.SdfParams(a.radius, a.half_width), fs.SdfSurface(1, 0, a.influence)
    for n in a.n:
        res = {"n": n, "dims": list(DIMS), "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "radius": a.radius, "half_width": a.half_width,
               "influence": a.influence, "runs": {m: [] for m in MODES}}
        for k in range(a.runs):
            for m in MODES:
                r = run(fs, fd, n, a.ppc, m, a.steps, a.warmup, prm, sf)
                res["runs"][m].append(r)
                print(f"n={n} run {k} {m:8s} {r['ms_per_step']:9.3f} ms/step  {json.dumps({x: y for x, y in r.items() if x not in ('mode', 'ms_per_step')})}", flush=True)
        med = {m: sorted(x["ms_per_step"] for x in v)[len(v) // 2] for m, v in res["runs"].items()}
        res["summary"] = {"median_ms": med, "spheres_minus_none_ms": med["spheres"] - med["none"], "averaged_minus_none_ms": med["averaged"] - med["none"],
                          "none_spread_ms": max(x["ms_per_step"] for x in res["runs"]["none"]) - min(x["ms_per_step"] for x in res["runs"]["none"])}
        print(f"n={n} median ms/step: none {med['none']:.3f}  spheres {med['spheres']:.3f}  averaged {med['averaged']:.3f}  spheres - none "
              f"{med['spheres'] - med['none']:+.3f}  averaged - none {med['averaged'] - med['none']:+.3f} (spread of none {res['summary']['none_spread_ms']:.3f})", flush=True)
        with open(os.path.join(a.out, f"blocks_{n}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
