#!/usr/bin/env python3
"""What particle sources and sinks cost a decomposed run: python tools/source_cost_blocks.py [--n 128] [--ppc 8] [--steps 12] [--warmup 4] [--runs 3] [--modes none slots]

Wall ms per step of a 2 x 2 x 2 block run (threads of this process over the in-process transport, all blocks on ONE GPU):
  none    no slot set: the step must cost what it cost before the slots existed (this form runs on older trees too: it calls
          nothing new, so the same file measures the parent commit)
  slots   one ADD source (grid velocity, every step), one FILL source (every step) and one sink, each over a 20 x 5 x 20 box at
          4 per cell around the grid's centre column: the ADD box above the cube, the FILL box in its top, the sink through its
          lower part — all three across the cut planes
Each form `--runs` times in fresh handles; the figure is slots - none over the medians, beside the spread of `none`.  The eight
blocks share one GPU and the transport stages through the host, so the number says what the slots add to such a run and nothing
about scaling or about RCCL between real peers.  The result goes to profiles/sources/blocks_<n>.json (--tag: blocks_<n>_<tag>.json)."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (2, 2, 2)


def slot_boxes(n):
    m = int(round(n * 41 / 121))
    a = n // 2 - m // 2
    b = a + m - 1                       # water_cube_drop's cube covers the indices a..b on every axis
    c = n // 2
    x0, x1 = c - 10, c + 9
    return {"add": ((x0, b + 3, x0), (x1, b + 7, x1)), "fill": ((x0, b - 4, x0), (x1, b, x1)), "sink": ((x0, a, x0), (x1, a + 4, x1))}


def run(fs, fd, n, ppc, mode, steps, warmup):
    size = DIMS[0] * DIMS[1] * DIMS[2]
    pos = fs.water_cube_drop(n, ppc, seed=0)
    cuts = fd.partition_blocks(n, pos, DIMS)
    grp = fd.LocalGroup(size)
    sims = [None] * size
    bar = threading.Barrier(size)
    t = [0.0, 0.0]
    bx = slot_boxes(n)

    def work(r):
        try:
            return block(r)
        except BaseException:
            bar.abort()                 # nobody is left waiting at the barrier
            raise

    def block(r):
        sim = fd.DistFluidSim(n, DIMS, cuts, grp.comms[r])
        sims[r] = sim
        sim.upload_global(pos)
        for _ in range(warmup):
            sim.step()
        if mode == "slots":
            sim.set_source(0, bx["add"][0], bx["add"][1], 4, mode="add", every=1, vel=None, seed=1)
            sim.set_source(1, bx["fill"][0], bx["fill"][1], 4, mode="fill", every=1, vel=(0.0, -1.0, 0.0), seed=2)
            sim.set_sink(0, bx["sink"][0], bx["sink"][1])
        bar.wait()
        if r == 0:
            t[0] = time.perf_counter()
        for _ in range(steps):
            sim.step()
        bar.wait()
        if r == 0:
            t[1] = time.perf_counter()
        return sim.source_stats() if mode == "slots" else None

    try:
        res = grp.run(work)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    out = {"mode": mode, "ms_per_step": (t[1] - t[0]) / steps * 1e3}
    if mode == "slots":
        out["emitted_total"], out["removed_total"] = res[0]["emitted_total"], res[0]["removed_total"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128])
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["none", "slots"], choices=["none", "slots"])
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sources"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    fd = fs.load_dist()
    os.makedirs(a.out, exist_ok=True)
    for n in a.n:
        res = {"n": n, "dims": list(DIMS), "ppc": a.ppc, "steps": a.steps, "warmup": a.warmup, "boxes": slot_boxes(n), "runs": {m: [] for m in a.modes}}
        for k in range(a.runs):
            for m in a.modes:
                r = run(fs, fd, n, a.ppc, m, a.steps, a.warmup)
                res["runs"][m].append(r)
                print(f"n={n} run {k} {m:5s} {r['ms_per_step']:9.3f} ms/step  {json.dumps({x: y for x, y in r.items() if x not in ('mode', 'ms_per_step')})}", flush=True)
        med = {m: sorted(x["ms_per_step"] for x in v)[len(v) // 2] for m, v in res["runs"].items()}
        res["summary"] = {"median_ms": med}
        if "none" in med:
            v = [x["ms_per_step"] for x in res["runs"]["none"]]
            res["summary"]["none_min_ms"], res["summary"]["none_max_ms"] = min(v), max(v)
        if "none" in med and "slots" in med:
            res["summary"]["slots_minus_none_ms"] = med["slots"] - med["none"]
        print(f"n={n} " + json.dumps(res["summary"]), flush=True)
        name = f"blocks_{n}" + (f"_{a.tag}" if a.tag else "") + ".json"
        with open(os.path.join(a.out, name), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
