#!/usr/bin/env python3
"""bench.py — substeps/s of the PIC/FLIP step (fluid.cc:1378-1490) on MI355X.

One "step" = one fluid_step(): sort + P2G, flags/index, the pressure do..while (RHS/divergence,
matrix-free PCG, velocity update, error), FLIP gather + advect, on the synthetic
water_cube_drop scene, particles and fields resident in HBM.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Prints ONE JSON line (rank 0).  `roofline` is for the dominant kernel of the timed region (the
fused PCG search-update + 7-point apply, FLUID_PROF_PCG_SQ), measured live with hipEvent pairs on
the solver's stream.  A plain run sets up, warms up, times the K steps and prints the line; the
legs that take runs of their own (`cpu_baseline` = the oracle timed on the same state, the 128^3
config, the stencil micro-benchmark, the x0 = 0 iteration count, the 500-step long run, the
snow-MPM legs, `parity_at_size`) run only with --full.

--dump-outputs DIR writes what the timed path computed in its last step as DIR/<name>.npy
(float64; a fixed, seeded sample of the particles and of the pressure cells, < 64 MB in all).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); measured copy ceiling ~6300


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=256, help="cells per axis (BASELINE configs: 128, 256)")
    ap.add_argument("--ppc", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cg-tol", type=float, default=2.220446049250313e-16, help="PCG relative tolerance (reference: Eigen epsilon)")
    ap.add_argument("--flip-blend", type=float, default=1.0, help="1 = the reference's pure FLIP; BASELINE config 1 names 0.95 (PIC/FLIP blend, build extension)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-micro", action="store_true", help="skip the dense stencil micro-benchmark")
    ap.add_argument("--cpu-steps", type=int, default=3, help="oracle steps timed per cpu_baseline leg (1 thread, all cores)")
    ap.add_argument("--no-long-run", action="store_true", help="skip the 500-step drop -> splash -> pool run (long_run key)")
    ap.add_argument("--long-steps", type=int, default=500, help="steps of the long run (the reference's loop runs 500, fluid.cc:1368)")
    ap.add_argument("--no-mpm", action="store_true", help="skip the snow-MPM leg (`mpm` key; SURVEY 8(f) f4)")
    # N > 1 extras are OFF unless asked for: they run collectives after the timed region, and a rank that fails inside one (an
    # out-of-memory while building a second handle) must not be able to cost the run its headline line
    ap.add_argument("--weak-leg", action="store_true", help="N > 1: also run the weak-scaling leg (256 N^(1/3) cells per axis, decomposed solve)")
    ap.add_argument("--alt-mode", action="store_true", help="N > 1: also time the other form of the multi-GPU pressure block")
    ap.add_argument("--no-weak-leg", action="store_true", help=argparse.SUPPRESS)   # (accepted for older command lines: the legs are off by default)
    ap.add_argument("--no-alt-mode", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dist-solve", default="decomposed", choices=["auto", "decomposed", "replicated"],
                    help="multi-GPU pressure block (FLUID_DIST_*).  Default: the domain-decomposed solve, the one BASELINE configs[3] names; "
                         "auto = the library's own choice (replicates the pressure block below 384^3)")
    ap.add_argument("--force-dist", action="store_true", help="run the decomposed code path even with one rank (overhead check)")
    ap.add_argument("--sample-every", type=int, default=32, help="bracket every k-th PCG launch (and every k/8-th P2G / sort / G2P / solve) with a hipEvent pair; each record stalls the stream ~5-10 us")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline (CPU baselines, 128^3 config, stencil micro-benchmark, x0 = 0 iterations, "
                         "long run, snow-MPM, parity at size); the --no-* options above switch single legs off")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (particle and pressure samples, step stats) as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be >= 1")
    return a


DUMP_SEED = 20240901            # fixed: the same cells and particles are sampled in every run
DUMP_PARTICLES = 500_000        # 2 x 12 MB of float64 (x, y, z)
DUMP_CELLS = 2_000_000          # 16 MB of float64 pressure


def _sample(total, k):
    """Sorted indices of a fixed, seeded sample of k out of `total` (all of them when total <= k)."""
    if total <= k:
        return np.arange(total)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(total, size=k, replace=False))


def dump_outputs(out_dir, sim, last, dist, world, rank, n_global):
    """What the timed path computed in its last step, as a caller of it receives it: particle positions and velocities (a fixed
    sample when there are more than DUMP_PARTICLES), the pressure field at a fixed sample of cells (one GPU), and the step's stats.
    Every rank takes part (the decomposed path gathers the sampled particles by global id); rank 0 writes."""
    keys = ("dt_in", "dt_out", "error", "max_speed", "relres", "num_active", "outer_passes", "cg_iters", "cg_iters_last")
    arrays = {"step_stats": np.array([float(last[k]) for k in keys], dtype=np.float64)}
    if dist is None:
        pos, vel = sim.download_particles()
        sel = _sample(len(pos), DUMP_PARTICLES)
        arrays["positions"], arrays["velocities"] = pos[sel], vel[sel]
        del pos, vel
        pres = sim.field(entry.load_package().FIELD.PRESSURE).reshape(-1)
        arrays["pressure_sample"] = np.ascontiguousarray(pres[_sample(pres.size, DUMP_CELLS)], dtype=np.float64)
        del pres
    else:
        # particles by global id (= index in the uploaded array); the pressure lives in per-rank windows and is not dumped here
        pos, vel, ids = sim.download_local()
        keep = np.isin(ids, _sample(n_global, DUMP_PARTICLES))
        parts = [None] * world
        dist.all_gather_object(parts, (ids[keep].astype(np.int64), pos[keep], vel[keep]))
        if rank == 0:
            gid = np.concatenate([p[0] for p in parts])
            order = np.argsort(gid, kind="stable")
            arrays["positions"] = np.concatenate([p[1] for p in parts])[order]
            arrays["velocities"] = np.concatenate([p[2] for p in parts])[order]
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        for name, arr in arrays.items():
            np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))


def usable_cores():
    """Host cores this process may really use: the affinity mask, capped by the cgroup CPU quota (a GPU box hands each
    GPU slot a share of the host: 256 logical CPUs visible, ~16 usable) and by the physical core count."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
        except Exception:  # noqa: BLE001
            pass
    try:
        phys, pid, cid = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pid = line.split(":")[1].strip()
            elif line.startswith("core id"):
                cid = line.split(":")[1].strip()
                phys.add((pid, cid))
        if phys:
            n = min(n, len(phys))
    except Exception:  # noqa: BLE001
        pass
    return max(1, n)


def pmc_traffic(kernel, n, ppc):
    """HBM/fabric bytes per launch measured by separate rocprofv3 --pmc passes of this workload (see the file's "method")."""
    tj = next((q for q in (os.path.join(ROOT, "profiles", r, "pmc_traffic.json") for r in ("r04", "r03", "r02")) if os.path.exists(q)), None)
    if n != 256 or ppc != 8 or tj is None:
        return None
    table = json.load(open(tj))
    table = table.get("kernels_final", table)   # (round 2 wrapped the per-kernel table; tools/pmc_summary.py writes it bare)
    if kernel not in table:
        # template arguments added since the key was written (k_pcg_xr_l<double> -> k_pcg_xr_l<double, false>): same base name, same leading arguments
        base, args = kernel.split("<")[0], kernel.partition("<")[2].rstrip(">")
        cand = [k for k in table if k.split("<")[0].split(" ")[0] == base and k.partition("<")[2].startswith(args)]
        if len(cand) != 1:
            return None
        kernel = cand[0]
    return table[kernel].get("bytes_per_launch")


def mpm_pmc_traffic():
    """Fabric bytes per operator application of the scaled snow cone (k_mpm_apply_particles + k_mpm_apply_cells), from the newest
    profiles/r0N/mpm_pmc.txt (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/mpm_run.py 63 24 64; FETCH_SIZE doubled)."""
    for r in ("r04", "r03"):
        path = os.path.join(ROOT, "profiles", r, "mpm_pmc.txt")
        if not os.path.exists(path):
            continue
        tot, seen = 0.0, set()
        for line in open(path):
            f = line.split()
            if len(f) >= 3 and f[0] in ("k_mpm_apply_particles", "k_mpm_apply_cells") and f[1] in ("FETCH_SIZE", "WRITE_SIZE"):
                tot += float(f[2]) * 1e6
                seen.add((f[0], f[1]))
        if len(seen) >= 2:
            return tot, f"profiles/{r}/mpm_pmc.txt ({', '.join(sorted(a + ' ' + b for a, b in seen))})"
    return None, None


def stencil_microbench(fs, n, device):
    """Dense sweep q = A s over all n^3 cells, all-fluid interior (SURVEY.md 8d micro-benchmark), timed two ways:
    `cache_resident` = 50 back-to-back launches over ONE (s, q, flags) set (151 MB for fp32 at 256^3: it fits the 256 MiB
    Infinity Cache, so this is not an HBM figure), `hbm` = launches rotating over enough separate sets to exceed 1 GiB
    (every operand byte comes from HBM and goes back to it).  The roofline evidence for the north star's
    ">= 70 % of HBM on the pressure-stencil kernel" is the `hbm` leg."""
    out = {"footprint_hbm_leg_bytes": 1 << 30}
    for prec, T in (("fp64", 8), ("fp32", 4)):
        sim = fs.FluidSim(n=n, precision=prec, device=device)
        F = fs.FIELD
        solid = sim.field(F.SOLID)
        sim.upload_field(F.CONTAINER, (solid == 0).astype(np.float32))
        sim.flags_index()
        rng = np.random.default_rng(1)
        s = rng.uniform(-1, 1, size=(n, n, n)) * (solid == 0)
        sim.upload_field(F.SEARCH, s)
        algo = n ** 3 * (2 * T + 1)
        res = {"bytes_per_cell": 2 * T + 1, "bytes_per_launch": algo}
        rate = lambda ms: {"ms": ms, "achieved_GBs": algo / (ms * 1e-3) / 1e9, "frac_of_peak": algo / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        for name, mode in (("march", 0), ("tiled", 2)):
            sim.stencil_apply(reps=5, box=mode)
            leg = {"cache_resident": rate(sim.stencil_apply(reps=50, box=mode))}
            # four calls: the first runs on freshly allocated sets and reads 5-8 % low whatever the warm-up (an allocation effect, not the
            # kernel's: later calls get the same blocks back from the allocator; tools/stencil_state.py) — `hbm` is the MEDIAN of the
            # three calls after it, every call is kept beside it
            calls = [sim.stencil_apply_hbm(reps=56, box=mode, footprint_bytes=out["footprint_hbm_leg_bytes"]) for _ in range(4)]
            ms = sorted(c[0] for c in calls[1:])[1]
            leg["hbm"] = rate(ms)
            leg["hbm"]["sets"] = calls[0][1]
            leg["hbm"]["frac_of_peak_by_call"] = [algo / (c[0] * 1e-3) / 1e9 / HBM_PEAK_GBS for c in calls]
            leg["hbm_first_call"] = rate(calls[0][0])
            res[name] = leg
        out[prec] = res
        sim.close()
    return out


def long_run_phases(ts, boxes, its_by_step):
    """Split the drop -> splash -> pool run by what the active box does: `free_fall` until the box first widens in x or z
    (the cube keeps its footprint while it falls), `settled` from the first step after which the box never changes
    again, `splash` in between; per phase: steps, mean / max ms per step, substeps/s, PCG iterations and outer passes."""
    n = len(ts)
    ext = [(b[1][0] - b[0][0], b[1][2] - b[0][2]) for b in boxes]
    fall_end = next((i for i in range(1, n) if ext[i][0] > ext[0][0] + 2 or ext[i][1] > ext[0][1] + 2), n)
    settle = n
    while settle > fall_end and boxes[settle - 1] == boxes[n - 1]:
        settle -= 1
    out = {}
    for name, lo, hi in (("free_fall", 0, fall_end), ("splash", fall_end, settle), ("settled", settle, n)):
        if hi > lo:
            seg = np.asarray(ts[lo:hi])
            out[name] = {"steps": [lo, hi], "mean_ms": float(seg.mean()), "max_ms": float(seg.max()), "substeps_per_s": float(1e3 / seg.mean()),
                         "share_of_time": float(seg.sum() / np.sum(ts)), "cg_iters": int(sum(x[0] for x in its_by_step[lo:hi])),
                         "outer_passes": int(sum(x[1] for x in its_by_step[lo:hi]))}
    return out


def main():
    a = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1 or a.force_dist:
        import torch
        import torch.distributed as dist_mod
        dist = dist_mod
        torch.cuda.set_device(local_rank)
        if world == 1:   # --force-dist outside a launcher: a rendezvous of one
            for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", str(29600 + os.getpid() % 300))):
                os.environ.setdefault(k, v)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    fs = entry.load_package()

    n, ppc = a.n, a.ppc
    pos0 = fs.water_cube_drop(n, ppc, seed=a.seed)
    transport = None
    solve_mode = "single"
    if world == 1 and not a.force_dist:
        sim = fs.FluidSim(n=n, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend)
        sim.upload_particles(pos0)
    else:
        # ONE simulation cut into 3-D blocks (8 ranks: 2 x 2 x 2), one block per GPU (strong scaling)
        fd = fs.load_dist()
        dims = fd.default_dims(world)
        cuts = fd.partition_blocks(n, pos0, dims)
        import torch
        comm, err = None, ""
        try:
            comm = fd.RcclComm()          # ncclSend/Recv/AllReduce enqueued on the solver stream by the C++ host
        except Exception as e:            # noqa: BLE001
            err = str(e)
        # every rank must take the same transport: agree on whether the native RCCL communicator came up everywhere
        ok = torch.tensor([1 if comm is not None else 0], device="cuda", dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            transport = "rccl (native, stream-ordered)"
        else:
            if comm is not None:
                comm.close()
            comm = fd.TorchComm(mode="device", device=torch.device("cuda", local_rank))
            transport = f"torch.distributed nccl callbacks (native RCCL init failed on some rank: {err})"
        sim = fd.DistFluidSim(n, dims, cuts, comm, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend, dist_solve=a.dist_solve)
        sim.upload_global(pos0)

    def barrier():
        if dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(a.warmup):
        st0 = sim.step()
        if transport is not None:
            solve_mode = "replicated" if st0["paths"] & 8 else "decomposed"    # FLUID_PATH_DIST_*: what FLUID_DIST_AUTO picked
    # state at the start of the timed region, for the CPU leg (--full)
    cpu_state = None
    if a.full and rank == 0 and not a.no_cpu and world == 1 and not a.force_dist:
        p, v = sim.download_particles()
        cpu_state = (p, v, sim.dt)

    sim.profile_reset()
    sim.profile_enable(a.sample_every)
    barrier()
    t0 = time.perf_counter()
    stats = []
    for _ in range(a.steps):
        stats.append(sim.step())   # fluid_step() synchronises its stream before returning
    barrier()
    t1 = time.perf_counter()
    sim.profile_enable(0)
    per_rank_particles = None
    if transport is not None:
        import torch
        cnt = torch.zeros(world, device="cuda", dtype=torch.int64)
        cnt[rank] = sim.num_live()
        dist.all_reduce(cnt)
        per_rank_particles = [int(x) for x in cnt.tolist()]
    if transport is not None and stats:
        solve_mode = "replicated" if stats[0]["paths"] & 8 else "decomposed"
    elapsed = t1 - t0
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, sim, stats[-1], dist, world, rank, len(pos0))

    # N > 1: the same steps with the OTHER form of the multi-GPU pressure block, timed the same way, reported beside the
    # headline as `alt_mode` (no multi-GPU box is available to the builder: this is how both forms get measured)
    def all_ok(flag):
        """Every rank takes a leg or none does: MIN over the ranks of `this rank built its handle`."""
        import torch
        t = torch.tensor([1 if flag else 0], device="cuda", dtype=torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return int(t.item()) == 1

    def build_leg(make):
        """Construct and upload a leg's handle; (handle or None, error text).  No collective inside a rank-local try."""
        try:
            return make(), ""
        except Exception as e:  # noqa: BLE001
            return None, str(e)[:300]

    alt = None
    if (world > 1 or a.force_dist) and a.alt_mode:
        other = "replicated" if solve_mode == "decomposed" else "decomposed"
        def make_alt():
            h = fd.DistFluidSim(n, dims, cuts, comm, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend, dist_solve=other)
            h.upload_global(pos0)
            return h
        sim_alt, err_alt = build_leg(make_alt)
        if not all_ok(sim_alt is not None):
            if sim_alt is not None:
                sim_alt.close()
            alt = {"pressure_block": other, "error": err_alt or "another rank could not build the handle"}
            sim_alt = None
        try:
            if sim_alt is None:
                raise StopIteration
            for _ in range(a.warmup):
                sim_alt.step()
            barrier()
            c0 = time.perf_counter()
            st_alt = [sim_alt.step() for _ in range(a.steps)]
            barrier()
            el = time.perf_counter() - c0
            import torch
            t = torch.tensor([el], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
            alt = {"pressure_block": other, "value": a.steps / el, "unit": "substeps/s", "ms_per_step": el / a.steps * 1e3,
                   "cg_iters_total": sum(x["cg_iters"] for x in st_alt), "outer_passes_total": sum(x["outer_passes"] for x in st_alt)}
            sim_alt.close()
        except StopIteration:
            pass
        except Exception as e:  # noqa: BLE001
            alt = {"pressure_block": other, "error": str(e)[:300]}

    # N > 1: a WEAK-scaling leg beside the strong-scaling headline — the cells per GPU of the 256^3 workload kept fixed, i.e. a grid of
    # 256 N^(1/3) cells per axis (8 GPUs: BASELINE configs[4], 512^3 with 4 particles per cell; fewer GPUs: 8 per cell), decomposed solve
    weak = None
    if (world > 1 or a.force_dist) and a.weak_leg and n == 256:
        nw = int(round(256 * world ** (1.0 / 3.0) / 8.0)) * 8
        ppcw = 4 if nw >= 512 else 8
        posw = fs.water_cube_drop(nw, ppcw, seed=a.seed)
        def make_weak():
            cutsw = fd.partition_blocks(nw, posw, dims)
            h = fd.DistFluidSim(nw, dims, cutsw, comm, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend, dist_solve="decomposed")
            h.upload_global(posw)
            return h
        simw, err_w = build_leg(make_weak)
        if not all_ok(simw is not None):
            if simw is not None:
                simw.close()
            weak = {"error": err_w or "another rank could not build the handle"}
            simw = None
        try:
            if simw is None:
                raise StopIteration
            for _ in range(a.warmup):
                simw.step()
            barrier()
            c0 = time.perf_counter()
            stw = [simw.step() for _ in range(a.steps)]
            barrier()
            el = time.perf_counter() - c0
            import torch
            t = torch.tensor([el], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
            weak = {"workload": f"water_cube_drop {nw}^3 grid, {ppcw} particles/cell, {len(posw)} particles, decomposed solve", "grid": nw,
                    "cells_vs_256": nw ** 3 / 256.0 ** 3, "value": a.steps / el, "unit": "substeps/s", "ms_per_step": el / a.steps * 1e3,
                    "cg_iters_total": sum(x["cg_iters"] for x in stw), "num_active_last": stw[-1]["num_active"],
                    "note": "one GPU runs 512^3 / 4 per cell at 71 substeps/s (profiles/r03/bench_512.json)"}
            simw.close()
        except StopIteration:
            pass
        except Exception as e:  # noqa: BLE001
            weak = {"error": str(e)[:300]}
        del posw

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    ms_per_step = elapsed / a.steps * 1e3
    # N>1: the SAME global problem on N GPUs -> strong scaling; value = steps of that one simulation per second
    value = a.steps / elapsed

    T = 8
    sq = sim.profile_read(fs.PROF.PCG_SQ)
    xr = sim.profile_read(fs.PROF.PCG_XR)
    solve = sim.profile_read(fs.PROF.SOLVE)
    p2g = sim.profile_read(fs.PROF.P2G)
    g2p = sim.profile_read(fs.PROF.G2P)
    srt = sim.profile_read(fs.PROF.SORT)
    mgs = sim.profile_read(fs.PROF.MG_UP0)
    # ---- roofline: every kernel class bracketed by hipEvents in the timed region, the one with the largest total
    # time in `roofline`, the others in `roofline_others`.  Algorithmic bytes per launch:
    #   k_p2g_rows    96 B per particle staged once (9 axis weights + 3 velocity components) + 52 B per cell written
    #   up leg, lvl 0 21.5 B/cell: read u (float), r (double), count byte, 1/8 coarse value (float); write z (double)
    #   SQ            33 B/cell: read z, s, count byte; write s', q          XR   49 B/cell: read x, r, s, q, count; write x, r
    np_ = float(len(pos0))
    def roof_entry(name, prof, bytes_fn, key, note=None):
        if not prof.get("sampled"):
            return None
        avg_ms = prof["total_ms"] / prof["sampled"]
        cells = prof["cells"] / prof["sampled"]
        algo = bytes_fn(cells)
        ach = algo / (avg_ms * 1e-3) / 1e9
        e = {"bound": "hbm", "kernel": name, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
             "traffic": pmc_traffic(key, n, ppc) if transport is None else None,
             "traffic_source": "profiles/r0N/pmc_traffic.json (newest round present): separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload, FETCH_SIZE doubled (gfx950)", "algorithmic_bytes_per_launch": algo,
             "cells_per_launch": cells, "avg_launch_us": avg_ms * 1e3, "launches": prof["launches"], "sampled": prof["sampled"],
             "total_ms_in_timed_region": avg_ms * prof["launches"]}
        if note:
            e["note"] = note
        return e
    small = ("the level-0 working set of this scene (~0.7 M cells, 6 MB per vector) lives in L2/Infinity Cache and the launch is "
             "latency-bound (~3 us of it is dispatch), so the HBM fraction is low by construction; the bandwidth-bound kernel of "
             "this path is the dense 256^3 stencil sweep (stencil_microbench)")
    cands = [
        roof_entry("k_p2g_rows<true> + k_p2g_combine (particle -> grid gather: a block marches over the source rows of one x-plane, "
                   "each row staged through LDS once; three x-plane partials per cell)", p2g,
              lambda c: np_ * 96 + c * 52, "k_p2g_rows<true>",
              "algorithmic bytes: 96 B per particle (9 axis weights + velocity) read once + 52 B per cell written; `traffic` (k_p2g_rows "
              "alone) adds the two halo rows per 12-column segment (x1.17) and the 3 x 32 B per cell of partials that k_p2g_combine "
              "reads back; the time is hipEvents around both kernels; bound by staging latency (stage -> barrier -> gather per row "
              "with 4 blocks per CU), not by bandwidth, DESIGN.md 3"),
        roof_entry("k_mg_up<float, double, double, 8, 8, 16> (level-0 up leg of the V-cycle: prolongation + two damped-Jacobi sweeps + r.z partials)",
              mgs, lambda c: c * 21.5, "k_mg_up<float, double, double, 8, 8, 16>", small),
        roof_entry("k_pcg_sq_l<double, false> (PCG: s' = z + beta s, q = A s', partial s'.q)", sq, lambda c: c * 33.0, "k_pcg_sq_l<double, false>", small),
        roof_entry("k_pcg_xr_l<double> (PCG: x += alpha s, r -= alpha q, partial r.r)", xr, lambda c: c * 49.0, "k_pcg_xr_l<double>", small),
    ]
    cands = [c for c in cands if c]
    cands.sort(key=lambda c: -c["total_ms_in_timed_region"])
    roof = cands[0] if cands else None
    roof_others = cands[1:]

    def per(d):
        return None if not d["sampled"] else d["total_ms"] / d["sampled"]

    out = {
        "metric": "simulated substeps/sec", "value": value, "unit": "substeps/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"water_cube_drop {n}^3 grid, {ppc} particles/cell, {len(pos0)} particles, " + ("pure FLIP" if a.flip_blend >= 1 else f"PIC/FLIP blend {a.flip_blend}"),
                   "grid": n, "ppc": ppc, "particles": int(len(pos0)), "cg_tol": a.cg_tol,
                   "parallelism": "single GPU" if transport is None else
                   (f"{dims[0]} x {dims[1]} x {dims[2]} blocks, one per GPU (cuts {cuts}); particles sharded (sort, migration, ghosts, P2G, G2P, advect); " +
                    ("window arrays = block + 4 halo cells, halo exchanges, domain-decomposed PCG with the globally coupled V-cycle" if solve_mode == "decomposed"
                     else "P2G fields all-reduced, pressure block replicated on every GPU") + f"; transport {transport}")},
        "roofline": roof,
        "roofline_others": roof_others,
        **({"pressure_block": solve_mode,
            "pressure_block_note": "value = ONE simulation on N GPUs with the pressure block in this form; decomposed (the default with N > 1) is the domain "
                                   "decomposition BASELINE configs[3] names; --dist-solve replicated / auto and --alt-mode time the other form",
            "particles_per_rank_last": per_rank_particles, "alt_mode": alt, "weak_leg": weak} if world > 1 or a.force_dist else {}),
        "step_stats": {"num_active_last": stats[-1]["num_active"], "outer_passes_total": sum(s["outer_passes"] for s in stats),
                       "cg_iters_total": sum(s["cg_iters"] for s in stats), "relres_last": stats[-1]["relres"],
                       "cg_iters_note": "solves start from the previous pressure (FLUID_START_WARM): not the reference's x0 = 0 count, see cg_iters_total_x0_zero",
                       "box_last": [stats[-1]["box_lo"], stats[-1]["box_hi"]]},
        "kernel_ms": {"mg_up0_avg": per(mgs) if mgs.get("sampled") else None, "pcg_sq_avg": per(sq), "pcg_xr_avg": per(xr), "solve_avg": per(solve), "p2g_avg": per(p2g),
                      "g2p_avg": per(g2p), "sort_avg": per(srt)},
    }

    # --full: everything below adds keys beside the headline; a failure there is recorded, the line is printed regardless.
    def aux_legs():
        if not a.no_micro and world == 1 and n == 256 and ppc == 8 and a.flip_blend >= 1:
            # BASELINE.json configs[1] taken literally (128^3, 8 particles/cell, FLIP blend 0.95), same metric, for reference
            # beside the 256^3 line above (the metric names both sizes; `value` is the larger one)
            sim1 = fs.FluidSim(n=128, device=local_rank, cg_tol=a.cg_tol, flip_blend=0.95)
            sim1.upload_particles(fs.water_cube_drop(128, 8, seed=a.seed))
            for _ in range(a.warmup):
                sim1.step()
            c0 = time.perf_counter()
            it1 = 0
            for _ in range(a.steps):
                it1 += sim1.step()["cg_iters"]
            c1 = time.perf_counter()
            out["other_configs"] = {"128^3, 8 particles/cell, PIC/FLIP blend 0.95 (BASELINE configs[1])":
                                    {"value": a.steps / (c1 - c0), "unit": "substeps/s", "ms_per_step": (c1 - c0) / a.steps * 1e3,
                                     "steps": a.steps, "cg_iters_total": it1}}
            sim1.close()

        if not a.no_micro and world == 1:
            out["stencil_microbench"] = {"workload": f"dense {n}^3 all-fluid interior, q=A s", **stencil_microbench(fs, n, local_rank)}
            if n != 128:
                # the metric names 128^3 as well: 2.1 M cells, 19 / 36 MB per set — one launch is ~5-10 us, launch-latency-bound
                out["stencil_microbench"]["at_128"] = {"workload": "dense 128^3 all-fluid interior, q=A s", **stencil_microbench(fs, 128, local_rank)}

        if not a.no_micro and world == 1:
            # the same timed steps with every solve started from x0 = 0 like the reference's cg.solve(b) (fluid.cc:1474): the
            # iteration count comparable with the reference's
            simz = fs.FluidSim(n=n, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend, solve_start="zero")
            simz.upload_particles(pos0)
            for _ in range(a.warmup):
                simz.step()
            out["step_stats"]["cg_iters_total_x0_zero"] = sum(simz.step()["cg_iters"] for _ in range(a.steps))
            simz.close()

        if not a.no_long_run and world == 1:
            # the reference's whole run: 500 steps (fluid.cc:1368) through drop -> splash -> settled pool; the headline above
            # times the free fall only
            siml = fs.FluidSim(n=n, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend)
            siml.upload_particles(pos0)
            ts, its, passes, boxes, its_by_step = [], 0, 0, [], []
            forms = {"p2g_tile_form": 0, "p2g_crowded_cells_on_mfma": 0, "tile_lists": 0, "droplets_solved_apart": 0, "galerkin_coarse_levels": 0}   # steps that took each form (stats.paths bits 1, 16, 2, 64, 128)
            for _ in range(a.long_steps):
                c0 = time.perf_counter()
                st = siml.step()
                ts.append((time.perf_counter() - c0) * 1e3)
                its += st["cg_iters"]; passes += st["outer_passes"]
                forms["p2g_tile_form"] += bool(st["paths"] & 1); forms["p2g_crowded_cells_on_mfma"] += bool(st["paths"] & 16); forms["tile_lists"] += bool(st["paths"] & 2); forms["droplets_solved_apart"] += bool(st["paths"] & 64); forms["galerkin_coarse_levels"] += bool(st["paths"] & 128)
                boxes.append((tuple(st["box_lo"]), tuple(st["box_hi"]))); its_by_step.append((st["cg_iters"], st["outer_passes"]))
            ts = np.array(ts)
            # phases of the run by the active box: free fall (the cube has not reached the floor: the box is still the cube's), splash (the box
            # grows), settled (from the step after which the box no longer changes)
            out["long_run_phases"] = long_run_phases(ts, boxes, its_by_step)
            out["long_run"] = {"steps": a.long_steps, "mean_ms": float(ts.mean()), "p95_ms": float(np.percentile(ts, 95)), "max_ms": float(ts.max()),
                               "total_s": float(ts.sum() / 1e3), "substeps_per_s": float(a.long_steps / (ts.sum() / 1e3)),
                               "mean_ms_by_100": [float(ts[i:i + 100].mean()) for i in range(0, a.long_steps, 100)],
                               "cg_iters_total": its, "outer_passes_total": passes, "box_last": [st["box_lo"], st["box_hi"]],
                               "num_active_last": st["num_active"], "steps_by_form": forms, "droplets_last": int(len(siml.droplets()))}
            siml.close()
            # the whole-run rate beside the headline (`value` stays on the BASELINE window: steps after the warm-up, free fall)
            out["value_long_run"] = out["long_run"]["substeps_per_s"]
            out["value_long_run_note"] = f"substeps/s over all {a.long_steps} steps of the drop -> splash -> settled pool run (long_run); value = the timed window after the warm-up (free fall)"

        if not a.no_mpm and world == 1:
            # the reference's second program (./run.sh mpm): its own scene (31^3 grid, 6205 particles) and a
            # scaled cone; the CPU figure beside it is the restatement (which hoists the per-particle SVDs the reference
            # repeats for each of its 729 node pairs — the reference itself is slower than this)
            def mpm_leg(B, layers, ppv, steps, warm):
                sim = fs.MpmSim(B=B, W=B - 2, device=local_rank)
                posm = fs.snow_cone(B=B, W=B - 2, layers=layers, points_per_voxel=ppv, seed=a.seed)
                sim.upload_particles(posm)
                for _ in range(warm):
                    sim.step()
                c0 = time.perf_counter()
                sts = [sim.step() for _ in range(steps)]
                sec = time.perf_counter() - c0
                d = {"grid": f"{2 * B + 1}^3", "particles": sim.num_particles, "steps": steps, "value": steps / sec, "unit": "steps/s",
                     "ms_per_step": sec / steps * 1e3, "num_active_last": sts[-1]["num_active"],
                     "cg_iters_mean": float(np.mean([x["cg_iters"] for x in sts])), "cg_error_max": float(max(x["cg_error"] for x in sts)),
                     "phase_ms": {k[3:]: float(np.mean([x[k] for x in sts])) for k in ("ms_transfer", "ms_forces", "ms_solve", "ms_deform", "ms_advect")},
                     "apply_kernel_us": float(np.mean([x["ms_apply_avg"] for x in sts]) * 1e3)}
                # One operator application = k_mpm_apply_particles (per particle: gather of G over its 8 weighted nodes from the node-indexed
                # operand, energy Hessian, A_p F_p^T: 66 doubles read, 10 written) + k_mpm_apply_cells (per non-empty cell: the sums onto its 8
                # corner nodes, 22 doubles read per particle).  Measured on the
                # fabric: the PMC bytes of the two kernels (139 MB per application on the scaled cone) are 0.8 of these algorithmic bytes, so the operator
                # streams the particle state once per application — bound by the memory side, priced against the HBM peak; the fp64 VECTOR peak
                # (78.6 TFLOP/s) is given beside it.
                # flops per particle, counted from the source (8 nodes x 24 + three 3x3 products + Hessian ~300 + 8 corners x 30): ~800
                flops = 800.0 * sim.num_particles
                us = d["apply_kernel_us"]
                cache_bytes = (66.0 + 10.0 + 22.0) * 8 * sim.num_particles
                d["roofline"] = {"kernel": "k_mpm_apply_particles + k_mpm_apply_cells (one application of the matrix-free operator; time = HIP events around both)",
                                 "bound": "hbm", "achieved": cache_bytes / (us * 1e-6) / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": cache_bytes / (us * 1e-6) / 8e12,
                                 "fp64_TFLOPs": flops / (us * 1e-6) / 1e12, "fp64_frac_of_78.6": flops / (us * 1e-6) / 78.6e12,
                                 "traffic": mpm_pmc_traffic()[0] if B == 63 else None, "traffic_source": mpm_pmc_traffic()[1] if B == 63 else None,
                                 "algorithmic_bytes_per_application": cache_bytes,
                                 "note": "98 doubles per particle and application (66 read + 10 written by the particle kernel, 22 read by the cell kernel); `traffic` = the fabric-side PMC bytes; the small "
                                         "scene is pure launch latency; per-kernel times and the PMC traffic: profiles/r04/mpm_*; "
                                         "sums are gathers in a fixed order (no atomics): two runs give the same bits"}
                sim.close()
                return d, posm
            try:
                out["mpm"], posm = mpm_leg(15, 4, 400.0, 100, 5)
                out["mpm"]["workload"] = "the reference's scene: cone of 16 voxels x 400 points, mt19937(0), v = (0, -50, 0) (mpm.cc:1037-1052,1277,484)"
                out["mpm_scaled"], _ = mpm_leg(63, 24, 64.0, 20, 2)
                out["mpm_scaled"]["workload"] = "cone of 24 layers x 64 points per voxel on a 127^3 grid"
                if not a.no_cpu:
                    from oracle import mpm_oracle as mo
                    orc = mo.MpmOracle()
                    orc.set_particles(posm)
                    orc.step()
                    c0 = time.perf_counter()
                    for _ in range(3):
                        orc.step()
                    sec = (time.perf_counter() - c0) / 3
                    try:
                        mpm_cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
                    except Exception:  # noqa: BLE001
                        mpm_cpu = ""
                    out["mpm"]["cpu_baseline"] = {"value": 1.0 / sec, "unit": "steps/s", "cores": 1, "cores_usable": usable_cores(), "kind": "port",
                                                  "cpu_model": mpm_cpu, "seconds": sec * 3,
                                                  "sample": "3 steps of the restatement (oracle/mpm_oracle.cpp; serial like mpm.cc, whose only threads are "
                                                            "the TBB particle loops it inherits from fluid.cc) on the reference's scene after one warm-up step"}
            except Exception as e:  # noqa: BLE001 — an auxiliary leg must not cost the headline line
                out.setdefault("mpm", {})["error"] = str(e)[:300]

        if cpu_state is not None:
            oracle = entry.load_oracle()
            # The reference's CPU path = TBB particle loops on all cores (fluid.cc:845,978,1126) + serial grid sweeps + serial
            # Eigen IC-PCG (fluid.cc:1352,1473-1474; run.sh has no -fopenmp).  When the build of the reference's vendored Eigen
            # travelled with the repo (oracle/_ref), the oracle's solves go through it.
            use_ref = oracle.ref_lib() is not None
            ncores = usable_cores()
            cpu_model = ""
            try:
                cpu_model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
            except Exception:  # noqa: BLE001
                pass
            solver = ("pressure solves by the reference's own vendored Eigen 3.3.4 ConjugateGradient<IncompleteCholesky> (oracle/_ref)"
                      if use_ref else "pressure solves by the restated Jacobi-CG (oracle/_ref not present)")

            def cpu_leg(threads):
                orc = oracle.Oracle(n=n, use_ref_solver=use_ref)
                if not use_ref:
                    orc.set_cg_tol(a.cg_tol)
                if a.flip_blend < 1:
                    orc.set_flip_blend(a.flip_blend)
                orc.set_threads(threads)
                orc.set_particles(cpu_state[0], cpu_state[1])
                orc.dt = cpu_state[2]
                csec = 0.0
                for _ in range(a.cpu_steps):
                    c0 = time.perf_counter()
                    orc.step()
                    csec += time.perf_counter() - c0
                return orc, csec

            # threads of the all-cores leg: the usable count may still overstate what the box really schedules (a GPU slot's CPU
            # share is not always visible as a quota), so the threaded P2G is timed with a few counts and the fastest is taken
            cal = oracle.Oracle(n=n, use_ref_solver=use_ref)
            cal.set_particles(cpu_state[0], cpu_state[1])
            best = (None, 1)
            for tcount in sorted({t for t in (8, 16, 32, 64, ncores) if t <= ncores}):
                cal.set_threads(tcount)
                c0 = time.perf_counter()
                cal.p2g()
                dtc = time.perf_counter() - c0
                if best[0] is None or dtc < best[0]:
                    best = (dtc, tcount)
            del cal
            nthreads = best[1]
            orc1, sec1 = cpu_leg(1)
            orcn, secn = cpu_leg(nthreads)
            sample = (f"{a.cpu_steps} oracle steps of the same {n}^3 workload from the state at the start of the timed region; {solver}; "
                      f"host CPU: {cpu_model}, {ncores} cores usable (affinity {len(os.sched_getaffinity(0))}, capped by the cgroup CPU quota and the physical core count)")
            out["cpu_baseline"] = {"value": a.cpu_steps / secn, "unit": "substeps/s", "cores": nthreads, "cores_usable": ncores, "kind": "port", "cpu_model": cpu_model,
                                   "seconds": secn, "sample": sample + " — particle loops on all cores under per-cell locks (the reference's TBB loops), grid sweeps and the Eigen solve serial like the reference's"}
            out["cpu_baseline_1thread"] = {"value": a.cpu_steps / sec1, "unit": "substeps/s", "cores": 1, "kind": "port", "cpu_model": cpu_model,
                                           "seconds": sec1, "sample": sample + " — one thread"}
            csteps, orc = a.cpu_steps, orc1
            # full-size parity readout: GPU vs oracle after the same number of steps from the same state
            sim2 = fs.FluidSim(n=n, device=local_rank, cg_tol=a.cg_tol, flip_blend=a.flip_blend)
            sim2.upload_particles(cpu_state[0], cpu_state[1])
            sim2.dt = cpu_state[2]
            for _ in range(csteps):
                sim2.step()
            pg, vg = sim2.download_particles()
            po, vo = orc.particles()
            out["parity_at_size"] = {"steps": csteps, "pos_rel_l2": float(np.linalg.norm(pg - po) / np.linalg.norm(po)),
                                     "vel_rel_l2": float(np.linalg.norm(vg - vo) / max(np.linalg.norm(vo), 1e-300)),
                                     "indices_equal": bool(np.array_equal(sim2.field(fs.FIELD.INDICES), orc.field(4)))}
            sim2.close()
    if a.full:
        try:
            aux_legs()
        except Exception as e:  # noqa: BLE001
            out["aux_error"] = f"{type(e).__name__}: {e}"[:400]
    if "value_long_run" in out:   # keep it next to `value` at the top of the line
        out = {k: out[k] for k in (["metric", "value", "value_long_run"] + [k for k in out if k not in ("metric", "value", "value_long_run")])}
    print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
