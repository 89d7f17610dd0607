#!/usr/bin/env python3
"""What one iteration of each level-set filter kind costs on the device, beside one box iteration, on the same scene and handle:
python tools/flow_cost.py [--n 256] [--ppc 8] [--warmup 5] [--runs 5] [--iters 16] [--radius 1.5] [--half-width 2.5]

The scene of tools/smooth_cost.py after `--warmup` steps, one handle.  Per kind (box W = 1, median W = 1, median W = 2, laplacian,
curvature) the wall time of fluid_sdf_snapshot_filtered + fluid_sdf_wait, untracked, with K = `--iters` iterations and with K = 0 plus
a dummy offset (the same front half, pack and copy, one launch instead of the passes); their difference over `--iters` is one
iteration: three launches for the box filter, one for a flow.  The kinds are alternated `--runs` times and the medians taken; the
first round is a warm-up and is dropped.  Reported per iteration: microseconds, and nanoseconds per leaf of the range (the
particles' base-cell box dilated by 4 cells, which is what a pass launches a block for) and per listed leaf."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [("box", 1), ("median", 1), ("median", 2), ("laplacian", 1), ("curvature", 1)]


def leaves_in_range(pos, n):
    lo = -(n // 2)
    hi = lo + n - 1
    L0 = lo & ~7
    c = np.where(pos >= 0, np.floor(pos + 0.5), np.ceil(pos - 0.5)).astype(np.int64)
    c = c[((c >= lo) & (c <= hi)).all(axis=1)]
    k = 1
    for a in range(3):
        c0, c1 = max(int(c[:, a].min()) - 4, lo), min(int(c[:, a].max()) + 4, hi)
        k *= ((c1 - L0) >> 3) - ((c0 - L0) >> 3) + 1
    return k


def timed(fs, sim, prm, filt):
    g = fs.SdfGridC()
    t0 = time.perf_counter()
    fs.check(fs.lib.fluid_sdf_snapshot_filtered(sim._h, C.byref(prm), C.byref(filt)))
    fs.check(fs.lib.fluid_sdf_wait(sim._h, C.byref(g)))
    return (time.perf_counter() - t0) * 1e3, g.n_leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--half-width", type=float, default=2.5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    fs = entry.load_package()
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    for _ in range(a.warmup):
        sim.step()
    pos, _ = sim.download_particles()
    in_range = leaves_in_range(np.asarray(pos, dtype=np.float64), a.n)
    prm = fs.SdfParams(a.radius, a.half_width)
    ms = {k: {"full": [], "empty": []} for k in KINDS}
    listed = 0
    for r in range(a.runs + 1):
        for kind, W in KINDS:
            sim.sdf_set_filter_kind(kind)
            full, listed = timed(fs, sim, prm, fs.SdfFilter(W, a.iters, 0.0))
            empty, _ = timed(fs, sim, prm, fs.SdfFilter(W, 0, 1e-3))
            if r > 0:                                     # (the first round allocates the second buffer and warms the caches)
                ms[(kind, W)]["full"].append(full)
                ms[(kind, W)]["empty"].append(empty)
    sim.close()
    res = {"n": a.n, "ppc": a.ppc, "warmup": a.warmup, "runs": a.runs, "iters": a.iters, "radius": a.radius, "half_width": a.half_width,
           "particles": int(len(pos)), "leaves_in_range": in_range, "leaves_listed": int(listed), "kinds": {}}
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    for (kind, W), v in ms.items():
        per_iter_us = (med(v["full"]) - med(v["empty"])) / a.iters * 1e3
        res["kinds"][f"{kind} W={W}"] = {"full_ms": med(v["full"]), "empty_ms": med(v["empty"]), "spread_full_ms": max(v["full"]) - min(v["full"]),
                                         "iteration_us": per_iter_us, "ns_per_leaf_in_range": per_iter_us * 1e3 / in_range,
                                         "ns_per_listed_leaf": per_iter_us * 1e3 / max(listed, 1)}
        print(f"n={a.n} {kind:9s} W={W}  K={a.iters}: {med(v['full']):8.3f} ms  K=0: {med(v['empty']):8.3f} ms  iteration {per_iter_us:9.2f} us  "
              f"{per_iter_us * 1e3 / in_range:8.1f} ns/leaf in range  {per_iter_us * 1e3 / max(listed, 1):8.1f} ns/listed leaf", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
