#!/usr/bin/env python3
"""What the averaged-position surface costs beside the spheres': python tools/avg_cost.py [--n 256] [--ppc 8] [--late 445] [--reps 7]
                                                                 [--radius 1.0] [--half-width 2.0]

One handle, the drop scene; on the state right after the upload and on the state `--late` steps leave (a settled pool), the wall
time of one level-set snapshot from the call to the end of its wait (the call reads the box and the count back and the wait ends
with the copy: both end in a device synchronise), in five forms that take turns `--reps` times after one round that sizes the buffers:
  spheres          fluid_sdf_snapshot, the union of spheres (R, w)
  averaged h=R+w   the same call under fluid_sdf_set_surface(AVERAGED, R + w)
  averaged h=4     and with the widest influence
  spheres + box    fluid_sdf_snapshot_filtered with the (W = 1, K = 4) box filter the averaged surface is meant to replace
  averaged + box   the same filter after the averaged search, for scale
Everything but the search is shared by the first three (bbox, count, scan, scatter, scan of the flags, pack, copy), so their
differences are the search's.  Leaves listed by each form are printed beside the times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def forms(a):
    hw = min(a.radius + a.half_width, 4.0)
    fl = [("spheres", ("spheres", None), None), (f"averaged h={hw:g}", ("averaged", hw), None), ("averaged h=4", ("averaged", 4.0), None),
          ("spheres + box(1,4)", ("spheres", None), (1, 4)), (f"averaged h={hw:g} + box(1,4)", ("averaged", hw), (1, 4))]
    return [f for k, f in enumerate(fl) if f[0] not in [g[0] for g in fl[:k]]]           # R + w = 4: one form less


def one(sim, a, surface, smooth):
    sim.sdf_set_surface(*surface)
    t0 = time.perf_counter()
    sim.sdf_snapshot(a.radius, a.half_width, smooth=smooth)
    g = sim.sdf_wait()
    return (time.perf_counter() - t0) * 1e3, g.n_leaves


def measure(sim, a, state, res):
    fl = forms(a)
    for name, surface, smooth in fl:                      # sizes the buffers, loads the code objects
        one(sim, a, surface, smooth)
    ms = {name: [] for name, _, _ in fl}
    leaves = {}
    for _ in range(a.reps):
        for name, surface, smooth in fl:
            t, k = one(sim, a, surface, smooth)
            ms[name].append(t)
            leaves[name] = k
    st = sim.sdf_stats()
    res[state] = {}
    for name, _, _ in fl:
        v = sorted(ms[name])
        res[state][name] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "leaves_listed": leaves[name]}
        print(f"n={a.n} {state:12s} {name:28s} {v[len(v) // 2]:9.3f} ms  ({v[0]:.3f} ... {v[-1]:.3f})  leaves {leaves[name]} / {st['leaves_in_grid']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--late", type=int, default=445)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--half-width", type=float, default=2.0)
    a = ap.parse_args()
    import __graft_entry__ as entry
    fs = entry.load_package()
    sim = fs.FluidSim(n=a.n)
    sim.upload_particles(fs.water_cube_drop(a.n, a.ppc, seed=0))
    res = {"n": a.n, "ppc": a.ppc, "late": a.late, "reps": a.reps, "radius": a.radius, "half_width": a.half_width, "particles": sim.num_particles}
    measure(sim, a, "after upload", res)
    for _ in range(a.late):
        sim.step()
    measure(sim, a, f"step {a.late}", res)
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
