#!/usr/bin/env python3
"""What surface attributes cost a decomposed run: python tools/attr_cost_blocks.py [--n 128 256] [--ppc 8] [--steps 12] [--warmup 4] [--runs 3]
                                                                               [--radius 1.5] [--half-width 2.5]

Wall ms per step of a 2 x 2 x 2 block run (threads of this process over the in-process transport, all blocks on ONE GPU), in four forms:
  none      no output
  surface   tools/sdf_cost_blocks.py's `surface`: fluid_dist_sdf_snapshot and fluid_dist_sdf_wait on every block after its step, the
            blocks' lists joined by fluid_sdf_grids_merge on a merger thread (two merge buffers in turn)
  attr      the same with rank records (include/fluid_hip.h, "liquid surface, attributes (decomposed runs)"):
            fluid_dist_sdf_snapshot_attr / fluid_dist_sdf_wait_attr and fluid_sdf_attr_grids_merge
  mesh_vel  `attr`, and the merger thread then meshes the merged list with vertex velocities (fluid_sdf_mesh, fluid_sdf_mesh_attr):
            the loop of `FLUID_BLOCKS=2x2x2 FLUID_BLOCKS_MESH=R,W FLUID_BLOCKS_MESH_VEL=1 ./run.sh fluid` without the file writes
For every form with output it also reports the merger's busy time per step, the sum over the ranks of the listed leaves against the
merged count, and the bytes that went to the host in the last step.  Each form `--runs` times in fresh handles; the summary is the
median.  The eight blocks share one GPU here, so the numbers say what the output adds to such a run and nothing about scaling over
real peers.  The result goes to profiles/attr/blocks_<n>.json."""
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
MODES = ("none", "surface", "attr", "mesh_vel")


class Merger(threading.Thread):
    """Joins the records of one step at a time; ctypes releases the GIL inside the library call."""

    def __init__(self, fs, size, n, attr, mesh):
        super().__init__(daemon=True)
        self.fs, self.size, self.n, self.attr, self.mesh = fs, size, n, attr, mesh
        self.cv = threading.Condition()
        self.job, self.done, self.quit, self.busy_s, self.mesh_s, self.leaves, self.vertices = None, 0, False, 0.0, 0.0, [], []
        self.buf = [None, None]
        self.vbuf = None

    def room(self, b, k):
        if self.buf[b] is None or len(self.buf[b][0]) < k:
            self.buf[b] = (np.empty((k + 64, 3), np.int32), np.empty((k + 64, 512), np.float32), np.empty((k + 64, 8), np.uint64),
                           np.empty((k + 64, 512), np.uint32), np.empty((k + 64, 3, 512), np.float32))
        return [x.ctypes.data_as(C.c_void_p) for x in self.buf[b]]

    def run(self):
        fs, lib = self.fs, self.fs.lib
        while True:
            with self.cv:
                self.cv.wait_for(lambda: self.job is not None or self.quit)
                if self.job is None:
                    return
                i, parts, recs = self.job
            t0 = time.perf_counter()
            if self.attr:
                k = lib.fluid_sdf_attr_grids_merge(parts, recs, self.size, 0, None, None, None, None, None)
            else:
                k = lib.fluid_sdf_grids_merge(parts, self.size, 0, None, None, None)
            assert k >= 0
            o, v, m, ids, vel = self.room(i & 1, k)
            if self.attr:
                assert lib.fluid_sdf_attr_grids_merge(parts, recs, self.size, k, o, v, m, ids, vel) == k
            else:
                assert lib.fluid_sdf_grids_merge(parts, self.size, k, o, v, m) == k
            t1 = time.perf_counter()
            self.busy_s += t1 - t0
            self.leaves.append(k)
            if self.mesh:
                p0 = parts[0]
                g = fs.SdfGridC(self.n, k, p0.background, p0.radius, p0.half_width, o if k else None, v if k else None, m if k else None)
                a = fs.SdfAttrC(k, ids if k else None, vel if k else None)
                nq = C.c_int64()
                nv = lib.fluid_sdf_mesh(C.byref(g), 0, 0, None, None, C.byref(nq))
                assert nv >= 0
                if self.vbuf is None or len(self.vbuf[0]) < nv or len(self.vbuf[1]) < nq.value:
                    self.vbuf = (np.empty((nv + 1024, 3), np.float32), np.empty((nq.value + 1024, 4), np.uint32), np.empty((nv + 1024, 3), np.float32))
                pv, pq, pw = (x.ctypes.data_as(C.c_void_p) for x in self.vbuf)
                if nv:
                    assert lib.fluid_sdf_mesh(C.byref(g), nv, nq.value, pv, pq, C.byref(nq)) == nv
                    assert lib.fluid_sdf_mesh_attr(C.byref(g), C.byref(a), nv, pw) == nv
                self.vertices.append(nv)
                self.mesh_s += time.perf_counter() - t1
            with self.cv:
                self.job, self.done = None, i + 1
                self.cv.notify_all()

    def submit(self, i, parts, recs):
        with self.cv:
            self.cv.wait_for(lambda: self.job is None)
            self.job = (i, parts, recs)
            self.cv.notify_all()

    def wait_done(self, k):
        with self.cv:
            self.cv.wait_for(lambda: self.done >= k)

    def stop(self):
        with self.cv:
            self.quit = True
            self.cv.notify_all()
        self.join()


def run(fs, fd, n, ppc, mode, steps, warmup, prm):
    size = DIMS[0] * DIMS[1] * DIMS[2]
    pos = fs.water_cube_drop(n, ppc, seed=0)
    cuts = fd.partition_blocks(n, pos, DIMS)
    grp = fd.LocalGroup(size)
    sims = [None] * size
    attr = mode in ("attr", "mesh_vel")
    parts = [(fs.SdfGridC * size)(), (fs.SdfGridC * size)()]
    recs = [(fs.SdfAttrPartC * size)(), (fs.SdfAttrPartC * size)()]
    listed = [[0] * size for _ in range(steps)]
    bar = threading.Barrier(size)
    mg = Merger(fs, size, n, attr, mode == "mesh_vel") if mode != "none" else None
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
            if mode == "none":
                continue
            if attr:
                fs.check(fs.lib.fluid_dist_sdf_snapshot_attr(sim._h, C.byref(prm)))
                fs.check(fs.lib.fluid_dist_sdf_wait_attr(sim._h, C.byref(parts[i & 1][r]), C.byref(recs[i & 1][r])))
            else:
                fs.check(fs.lib.fluid_dist_sdf_snapshot(sim._h, C.byref(prm)))
                fs.check(fs.lib.fluid_dist_sdf_wait(sim._h, C.byref(parts[i & 1][r])))
            listed[i][r] = parts[i & 1][r].n_leaves
            bar.wait()                          # every block's record of step i is in parts[i & 1]
            if r == 0:
                mg.submit(i, parts[i & 1], recs[i & 1])   # (waits for merge i - 1: the other half is free before step i + 1 ends)
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
        out["listed_over_merged"] = sum(sum(x) for x in listed) / max(1, sum(mg.leaves))
        out["merge_busy_ms_per_step"] = mg.busy_s / steps * 1e3
        out["bytes_to_host_last_step_all_blocks"] = int(sum(res))
        if mode == "mesh_vel":
            out["mesh_busy_ms_per_step"] = mg.mesh_s / steps * 1e3
            out["vertices_mean"] = sum(mg.vertices) / steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--half-width", type=float, default=2.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    fd = fs.load_dist()
    os.makedirs(a.out, exist_ok=True)
    prm = fs.SdfParams(a.radius, a.half_width)
    for n in a.n:
        res = {"n": n, "dims": list(DIMS), "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "radius": a.radius, "half_width": a.half_width,
               "runs": {m: [] for m in MODES}}
        for k in range(a.runs):
            for m in MODES:
                r = run(fs, fd, n, a.ppc, m, a.steps, a.warmup, prm)
                res["runs"][m].append(r)
                print(f"n={n} run {k} {m:8s} {r['ms_per_step']:9.3f} ms/step  {json.dumps({x: y for x, y in r.items() if x not in ('mode', 'ms_per_step')})}", flush=True)

        def median(m, key):
            v = sorted(x[key] for x in res["runs"][m])
            return v[len(v) // 2]
        med = {m: median(m, "ms_per_step") for m in MODES}
        none = [x["ms_per_step"] for x in res["runs"]["none"]]
        res["summary"] = {"median_ms": med, "none_spread_ms": max(none) - min(none),
                          "surface_minus_none_ms": med["surface"] - med["none"], "attr_minus_surface_ms": med["attr"] - med["surface"],
                          "mesh_vel_minus_attr_ms": med["mesh_vel"] - med["attr"],
                          "merge_busy_median_ms": {m: median(m, "merge_busy_ms_per_step") for m in MODES[1:]},
                          "bytes_to_host": {m: median(m, "bytes_to_host_last_step_all_blocks") for m in MODES[1:]}}
        print(f"n={n} median ms/step: " + "  ".join(f"{m} {med[m]:.3f}" for m in MODES) + f"  (spread of none {res['summary']['none_spread_ms']:.3f})  "
              f"merge busy {res['summary']['merge_busy_median_ms']}  bytes to host {res['summary']['bytes_to_host']}", flush=True)
        with open(os.path.join(a.out, f"blocks_{n}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
