"""GPU (-m gpu): the velocity trails of a decomposed run (include/fluid_hip.h, "liquid surface, velocity trails (decomposed runs)"):
the rank records of fluid_dist_sdf_snapshot_trails (k_trail_count<true>, k_trail_expand<true>) against tests/sdf_trail_ref.py of the
rank's downloaded live positions and velocities, and their merge (fluid_sdf_grids_merge as it is) against the reference of all
ranks' particles and against a one-GPU handle under fluid_sdf_set_trails.  Every comparison is exact: bit patterns of the values,
equality of masks and origins.  Blocks run as threads of a LocalGroup on the one GPU of the box; block, run_group and CASES are
those of tests/test_gpu_dist_sdf_avg.py, restated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import leaf_ref
import sdf_avg_ref
import sdf_ref
import sdf_trail_ref as ref
import vdb_reader
from sdf_testlib import FLUID, FLUID_VARS, same_grid, u32

pytestmark = pytest.mark.gpu

SETS = ref.SETS                                           # (R, w, dx): (3, 1, 1) for the inside rule, (1, 2, 0.5) for dx != 1
LEAF_BYTES = 2048 + 64 + 12                               # FLUID_SDF_LEAF_BYTES
ERR_ARG, ERR_STATE = 1, 3
REBALANCED = 32                                           # FLUID_PATH_DIST_REBALANCED
CASES = [                                                 # those of tests/test_gpu_dist_sdf.py
    (16, (2, 1, 1), (3, 3, 3)),
    (25, (2, 2, 1), (3, 3, 3)),          # odd N: the first leaf starts outside the grid
    (32, (2, 2, 2), (3, 3, 3)),          # the leaf around the corner of the eight blocks
    (24, (1, 1, 3), (2, 2, 6)),          # a middle block with a cut on either side
]
MORE_VARS = ("FLUID_OUT_SURFACE_KIND", "FLUID_BLOCKS_SURFACE_KIND", "FLUID_OUT_SURFACE_TRAILS", "FLUID_BLOCKS_SURFACE_TRAILS")


def block(h, ppc, seed, centre=(0, 0, 0)):
    """`ppc` points in every cell of [c - h, c + h) per axis."""
    rng = np.random.default_rng(seed)
    ax = [np.arange(centre[a] - h[a], centre[a] + h[a]) for a in range(3)]
    c = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.repeat(c, ppc, axis=0) + rng.uniform(-0.49, 0.49, (ppc * len(c), 3))


def velocities(pos, seed):
    """A random direction times uniform(0, 6) voxels per shutter."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=pos.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * rng.uniform(0.0, 6.0, (len(pos), 1))


def at_the_faces(n):
    """Four particles 0.8 voxels inside a face of the grid, moving inwards at 5 voxels per shutter: their trails leave the grid.
    (The block's own trails cannot at n = 16: they start within 3.5 voxels of the centre, are shorter than 6 voxels, and with
    R = 1 shorter than 3.5.)"""
    lo, hi, _, _ = sdf_ref.geometry(n)
    pos = np.array([[hi - 0.8, 0.2, 0.1], [lo + 0.8, -0.3, 0.2], [0.3, hi - 0.8, -0.4], [0.1, -0.2, lo + 0.8]])
    vel = np.array([[-5.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, -5.0, 0.0], [0.0, 0.0, 5.0]])
    return pos, vel


def run_group(fs, dims, n, cuts, work, **kw):
    """work(sim, r) on every rank of a LocalGroup; returns the results by rank."""
    fd = fs.load_dist()
    size = dims[0] * dims[1] * dims[2]
    grp = fd.LocalGroup(size)
    sims = [None] * size

    def run(r):
        sim = fd.DistFluidSim(n, dims, cuts, grp.comms[r], **kw)
        sims[r] = sim
        return work(sim, r)

    try:
        return grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()


def snap_trails(sim, R, w, t):
    sim.sdf_snapshot_trails(R, w, *t)
    return sim.sdf_wait()


def entries(fs, sim):
    """Entries of the handle's particle arrays, the dead ones included."""
    return int(fs.lib.fluid_num_particles(sim._h))


def check_dense(g, val, act, n, R, w, dx, what=""):
    """g is exactly the leaf list of the dense reference (val, act)."""
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert g.n == n and (g.background, g.radius, g.half_width) == (bg, fR, fw), what
    assert g.n_leaves == len(org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.origin, org), what
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what


def check_trails(g, pos, vel, n, R, w, dx, t, what=""):
    """g is exactly the leaf list of the reference's grid for the trails of (pos, vel).  Returns (values, active, instances)."""
    P, r, _ = ref.instances(pos, vel, R, t)
    val, act = ref.union(P, r, n, R, w, dx)
    check_dense(g, val, act, n, R, w, dx, what)
    return val, act, len(P)


def one_gpu(fs, pos, vel, n, R, w, dx, t):
    """fluid_sdf_snapshot under fluid_sdf_set_trails on one handle that holds (pos, vel)."""
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    sim.sdf_set_trails(*t)
    sim.sdf_snapshot(R, w)
    g = sim.sdf_wait()
    sim.close()
    return g


def view(gc):
    """(origins, values, mask words) of a fluid_sdf_grid_t as arrays over the handle's own pinned memory: no copy."""
    k = gc.n_leaves
    if k == 0:
        return np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 8), np.uint64)
    o = np.ctypeslib.as_array(C.cast(gc.origin, C.POINTER(C.c_int32)), shape=(k, 3))
    v = np.ctypeslib.as_array(C.cast(gc.values, C.POINTER(C.c_float)), shape=(k, 512))
    m = np.ctypeslib.as_array(C.cast(gc.active, C.POINTER(C.c_uint64)), shape=(k, 8))
    return o, v, m


def mask_words(active):
    """(k, 512) bool -> (k, 8) uint64: bit off & 63 of word off >> 6."""
    return np.packbits(np.asarray(active, dtype=bool).reshape(-1, 512), axis=1, bitorder="little").view(np.uint64).reshape(-1, 8)


def owner_cells(sim):
    """The rank's block as inclusive base-cell bounds per axis (edge blocks reach to infinity on their outer sides)."""
    lo = [sim.own_lo[a] + sim.lo if sim.own_lo[a] > 0 else -(1 << 60) for a in range(3)]
    hi = [sim.own_hi[a] + sim.lo - 1 if sim.own_hi[a] < sim.n else (1 << 60) for a in range(3)]
    return np.array(lo), np.array(hi)


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n,dims,hb", CASES, ids=[f"n{c[0]}" for c in CASES])
def test_rank_records_and_their_merge(fs, n, dims, hb, R, w, dx):
    fd = fs.load_dist()
    pos = block(hb, 2, n)
    vel = velocities(pos, n + 1)
    pos, vel = np.vstack([pos, at_the_faces(n)[0]]), np.vstack([vel, at_the_faces(n)[1]])
    t = ref.trails_of(R)
    lo, hi, _, nl = sdf_ref.geometry(n)

    def work(sim, r):
        sim.upload_global(pos, vel)
        blo, bhi = owner_cells(sim)
        out = []
        for k in range(4):
            if k:
                sim.step()
            g = snap_trails(sim, R, w, t)
            p, v, _ = sim.download_local()
            _, _, made = check_trails(g, p, v, n, R, w, dx, t, (r, k))
            st, ts = sim.sdf_stats(), sim.sdf_dist_trails_stats()
            print(f"rank {r} snapshot {k}: live {len(p)} entries {entries(fs, sim)} instances {made} leaves {g.n_leaves} stats {st} {ts}")
            assert st == {"leaves_in_grid": nl ** 3, "leaves_listed": g.n_leaves, "bytes_to_host": g.n_leaves * LEAF_BYTES + 4}, (r, k)
            assert ts == {"particles": len(p), "instances": made}, (r, k)
            c = sdf_ref.base_cell(ref.instances(p, v, R, t)[0])
            ingrid = ((c >= lo) & (c <= hi)).all(axis=1)
            abroad = ingrid & ~((c >= blo) & (c <= bhi)).all(axis=1)
            out.append(dict(g=g, p=p, v=v, dead=entries(fs, sim) - len(p), abroad=int(abroad.sum()), outside=int((~ingrid).sum())))
        return out

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dist_solve="decomposed", dx=dx)
    assert all(len(r[0]["p"]) > 0 for r in res)                            # the block straddles the cuts: every rank holds some
    assert max(r[0]["abroad"] for r in res) > 0                            # an instance whose base cell another rank owns
    assert max(r[0]["outside"] for r in res) > 0                           # an instance outside the grid (at n = 16 as at every n)
    for k in range(4):
        parts = [r[k]["g"] for r in res]
        allp, allv = np.concatenate([r[k]["p"] for r in res]), np.concatenate([r[k]["v"] for r in res])
        merged = fs.merge_sdf_grids(parts)
        check_trails(merged, allp, allv, n, R, w, dx, t, k)
        same_grid(merged, one_gpu(fs, allp, allv, n, R, w, dx, t), f"one GPU, snapshot {k}")
        assert sum(p.n_leaves for p in parts) > merged.n_leaves > 0          # a leaf near a cut is listed from both sides
        dead = [r[k]["dead"] for r in res]
        print(f"snapshot {k}: leaves per rank {[p.n_leaves for p in parts]} merged {merged.n_leaves} dead entries {dead} "
              f"abroad {[r[k]['abroad'] for r in res]} outside {[r[k]['outside'] for r in res]}")
        assert all(d == 0 for d in dead) if k == 0 else max(dead) > 0        # after a step the served ghosts are still in the arrays


@pytest.mark.parametrize("x", [-0.7, -0.3])
def test_a_trail_across_the_cut(fs, x):
    """One particle beside the cut of 2x1x1 at n = 16 with velocity (-5, 0, 0), shutter 1: the trail runs along +x into rank 1's
    half.  The other rank holds no live particle: the empty record, zero stats, no fault.  At x = -0.7 the particle is rank 0's
    (base cell -1) and every instance beyond instance 0 has its base cell in rank 1's block; at x = -0.3 the base cell is 0, the
    first cell of rank 1's block, so the particle and its whole trail are rank 1's and rank 0 is the empty one."""
    fd = fs.load_dist()
    n, dims, (R, w, dx) = 16, (2, 1, 1), SETS[1]
    t = ref.trails_of(R)
    pos, vel = np.array([[x, 0.2, 0.1]]), np.array([[-5.0, 0.0, 0.0]])
    P = ref.instances(pos, vel, R, t)[0]
    cells = sdf_ref.base_cell(P)[:, 0]
    assert len(P) > 3 and (cells[1:] >= 0).all()
    holder = 0 if x == -0.7 else 1
    assert (cells[0] < 0) == (holder == 0)

    def work(sim, r):
        sim.upload_global(pos, vel)
        g = snap_trails(sim, R, w, t)
        p, v, _ = sim.download_local()
        check_trails(g, p, v, n, R, w, dx, t, r)
        return g, p, v, sim.sdf_dist_trails_stats(), sim.sdf_stats()

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dx=dx)
    g, p, _, ts, st = res[1 - holder]
    assert len(p) == 0 and g.n_leaves == 0 and ts == {"particles": 0, "instances": 0} and st["leaves_listed"] == 0 and st["bytes_to_host"] == 4
    g, p, _, ts, _ = res[holder]
    assert len(p) == 1 and ts == {"particles": 1, "instances": len(P)}
    assert (g.origin[:, 0] >= 0).any()                                     # leaves of rank 1's half
    merged = fs.merge_sdf_grids([r[0] for r in res])
    check_trails(merged, pos, vel, n, R, w, dx, t)
    same_grid(merged, one_gpu(fs, pos, vel, n, R, w, dx, t), "one GPU")


def test_a_trail_from_outside_the_grid(fs):
    """The particle just outside the grid's +x face (base cell hi + 1: it does not count itself), the trail pointing inwards: the
    record of the rank that holds it is the surface of the in-grid instances."""
    fd = fs.load_dist()
    n, dims, (R, w, dx) = 16, (2, 1, 1), SETS[1]
    t = ref.trails_of(R)
    lo, hi, _, _ = sdf_ref.geometry(n)
    pos, vel = np.array([[hi + 0.6, 0.2, 0.1]]), np.array([[5.0, 0.0, 0.0]])
    P = ref.instances(pos, vel, R, t)[0]
    cells = sdf_ref.base_cell(P)[:, 0]
    assert cells[0] == hi + 1 and (cells[1:] <= hi).sum() > 2

    def work(sim, r):
        sim.upload_global(pos, vel)
        g = snap_trails(sim, R, w, t)
        p, v, _ = sim.download_local()
        _, act, _ = check_trails(g, p, v, n, R, w, dx, t, r)
        return g, p, sim.sdf_dist_trails_stats(), bool(act.any())

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dx=dx)
    assert len(res[0][1]) == 0 and res[0][0].n_leaves == 0 and res[0][2] == {"particles": 0, "instances": 0}
    assert len(res[1][1]) == 1 and res[1][0].n_leaves > 0 and res[1][3] and res[1][2] == {"particles": 1, "instances": len(P)}
    assert not sdf_ref.closed(pos, n, R, w, dx)[1].any()                   # the particle itself draws nothing
    merged = fs.merge_sdf_grids([r[0] for r in res])
    check_trails(merged, pos, vel, n, R, w, dx, t)


@pytest.mark.parametrize("swallow", [False, True], ids=["part", "a_whole_rank"])
def test_removed_particles_do_not_count(fs, swallow):
    """The sink scene of tests/test_gpu_dist_sdf.py with velocities: the records are of the survivors.  With the second sink box,
    which takes every cell from one before the cut upwards in x, every entry of rank 1 is dead and its record is empty."""
    fd = fs.load_dist()
    n, dims, (R, w, dx) = 24, (2, 1, 1), SETS[1]
    t = ref.trails_of(R)
    pos = block((4, 3, 3), 2, 5)
    vel = velocities(pos, 6) * 0.25                                        # (the step moves them: well below a cell per step)
    lo, hi = (9, 9, 9), (13, 14, 14)                                       # array indices: part of the block, across the cut at 12

    def work(sim, r):
        sim.upload_global(pos, vel)
        sim.set_sink(0, lo, hi)
        if swallow:
            sim.set_sink(1, (11, 0, 0), (23, 23, 23))
        sim.step()
        g = snap_trails(sim, R, w, t)
        p, v, _ = sim.download_local()
        _, _, made = check_trails(g, p, v, n, R, w, dx, t, r)
        assert sim.sdf_dist_trails_stats() == {"particles": len(p), "instances": made}, r
        return dict(g=g, p=p, v=v, dead=entries(fs, sim) - len(p), removed=sim.source_stats()["removed_last"])

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dist_solve="decomposed", dx=dx)
    p, v = np.concatenate([r["p"] for r in res]), np.concatenate([r["v"] for r in res])
    print([(len(r["p"]), r["dead"], r["removed"], r["g"].n_leaves) for r in res])
    assert res[0]["removed"] > 0 and len(p) == len(pos) - res[0]["removed"]
    assert all(r["dead"] > 0 for r in res)                                 # the removed particles (and ghosts) are still in the arrays
    if swallow:
        assert len(res[1]["p"]) == 0 and res[1]["g"].n_leaves == 0 and len(res[0]["p"]) > 0
    merged = fs.merge_sdf_grids([r["g"] for r in res])
    check_trails(merged, p, v, n, R, w, dx, t)
    assert merged.n_leaves > 0


@pytest.mark.parametrize("n", [16, 25])
def test_plain_handle_and_settings_untouched(fs, n):
    R, w, dx = SETS[1]
    A, B = (1.0, 1.0, R / 2, 8), (0.7, 1.5, R / 3, 5)
    pos = block((3, 3, 3), 2, n)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, velocities(pos, n + 1) * 0.5)
    sim.step()
    p, v = sim.download_particles()
    v = v * 8.0                                                            # (a settled step leaves them slow: one instance each)
    sim.upload_particles(p, v)
    assert sim.sdf_dist_trails_stats() == {"particles": 0, "instances": 0}  # before the first such snapshot
    gb = snap_trails(sim, R, w, B)
    _, _, made_b = check_trails(gb, p, v, n, R, w, dx, B, "B on a plain handle")
    assert made_b > len(p) and sim.sdf_dist_trails_stats() == {"particles": len(p), "instances": made_b}
    assert sim.sdf_trails_stats() == {"particles": 0, "instances": 0}       # the setting's counters are its own
    # under the handle's setting A the call still gives B, and the setting stays
    sim.sdf_set_trails(*A)
    sim.sdf_snapshot(R, w)
    ga = sim.sdf_wait()
    _, _, made_a = check_trails(ga, p, v, n, R, w, dx, A, "A, the setting")
    assert made_a != made_b
    before = sim.sdf_trails_stats()
    assert before == {"particles": len(p), "instances": made_a}
    same_grid(snap_trails(sim, R, w, B), gb, "B under the setting A")
    assert sim.sdf_trails_stats() == before
    sim.sdf_snapshot(R, w)
    same_grid(sim.sdf_wait(), ga, "A after B")
    # under AVERAGED likewise
    sim.sdf_set_trails(None)
    sim.sdf_set_surface("averaged", 3.0)
    sim.sdf_snapshot(R, w)
    avg = sim.sdf_wait()
    same_grid(snap_trails(sim, R, w, B), gb, "B under AVERAGED")
    sim.sdf_snapshot(R, w)
    same_grid(sim.sdf_wait(), avg, "AVERAGED after B")
    val, act = sdf_avg_ref.averaged(p, n, R, w, dx, 3.0)
    check_dense(avg, val, act, n, R, w, dx, "AVERAGED")
    # the ways back to the spheres' rank record
    sim.sdf_set_surface("spheres")
    gc = fs.SdfGridC()
    fs.check(fs.lib.fluid_dist_sdf_snapshot(sim._h, C.byref(fs.SdfParams(R, w))))
    fs.check(fs.lib.fluid_dist_sdf_wait(sim._h, C.byref(gc)))
    o, vals, m = (x.copy() for x in view(gc))
    for what, tt in (("max_instances = 1", (1.0, 1.0, R / 2, 1)), ("shutter 0", (0.0, 1.0, R / 2, 8))):
        g = snap_trails(sim, R, w, tt)
        assert g.n_leaves == len(o) > 0 and g.origin.tobytes() == o.tobytes() and g.values.tobytes() == vals.tobytes(), what
        assert mask_words(g.active).tobytes() == m.tobytes(), what
        assert sim.sdf_dist_trails_stats() == {"particles": len(p), "instances": len(p)}, what
    sim.close()


def test_slots_kinds_and_refusals(fs):
    n, (R, w, dx) = 16, SETS[1]
    pos = block((3, 3, 3), 2, 3)
    vel = velocities(pos, 4)
    t = ref.trails_of(R)
    sim = fs.FluidSim(n=n, dx=dx)
    hd = sim._h
    sim.upload_particles(pos, vel)
    prm, good, avg = fs.SdfParams(R, w), fs.SdfTrails(*t, 0), fs.SdfSurface(1, 0, 3.0)
    g, a = fs.SdfGridC(), fs.SdfAvgPartC()
    snap = lambda tr=good, p=prm: fs.lib.fluid_dist_sdf_snapshot_trails(hd, C.byref(p), C.byref(tr))   # noqa: E731
    nothing = lambda: fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == ERR_STATE                            # noqa: E731
    # bad arguments: refused, nothing outstanding
    assert fs.lib.fluid_dist_sdf_snapshot_trails(None, C.byref(prm), C.byref(good)) == ERR_ARG
    assert fs.lib.fluid_dist_sdf_snapshot_trails(hd, None, C.byref(good)) == ERR_ARG and nothing()
    assert fs.lib.fluid_dist_sdf_snapshot_trails(hd, C.byref(prm), None) == ERR_ARG and nothing()
    inf, nan = float("inf"), float("nan")
    for bad in ((-1.0, 1.0, 0.5, 8, 0), (inf, 1.0, 0.5, 8, 0), (nan, 1.0, 0.5, 8, 0), (1.0, 0.0, 0.5, 8, 0), (1.0, -1.0, 0.5, 8, 0), (1.0, inf, 0.5, 8, 0),
                (1.0, nan, 0.5, 8, 0), (1.0, 1.0, 0.0, 8, 0), (1.0, 1.0, -0.5, 8, 0), (1.0, 1.0, inf, 8, 0), (1.0, 1.0, nan, 8, 0), (1.0, 1.0, 0.5, 0, 0),
                (1.0, 1.0, 0.5, 33, 0), (1.0, 1.0, 0.5, -1, 0), (1.0, 1.0, 0.5, 8, 1)):
        assert snap(fs.SdfTrails(*bad)) == ERR_ARG and nothing(), bad
    assert snap(fs.SdfTrails(1.0, 1.0, R + 0.25, 8, 0)) == ERR_ARG and "radius_min" in fs.lib.fluid_last_error().decode() and nothing()
    assert snap(fs.SdfTrails(1.0, 1.0, R, 8, 0)) == 0 and fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == 0   # Rm = R is allowed
    for bad in ((2.0, 2.5), (1.5, 0.5), (0.0, 2.0), (nan, 2.0)):
        assert snap(p=fs.SdfParams(*bad)) == ERR_ARG and nothing(), bad
    assert fs.lib.fluid_dist_sdf_trails_stats(None, None, None) == ERR_ARG and fs.lib.fluid_dist_sdf_trails_stats(hd, None, None) == 0
    one = C.c_int64(-1)
    assert fs.lib.fluid_dist_sdf_trails_stats(hd, C.byref(one), None) == 0 and one.value == len(pos)
    assert fs.lib.fluid_dist_sdf_trails_stats(hd, None, C.byref(one)) == 0 and one.value > len(pos)
    # two outstanding, then FLUID_ERR_STATE; both waits of a plain record take it
    want = ref.trails_surface(pos, vel, n, R, w, dx, t)
    assert snap() == 0 and snap() == 0
    assert snap() == ERR_STATE and "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    check_dense(sim.sdf_wait(), *want, n, R, w, dx, "fluid_sdf_wait on a plain handle")
    assert fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == 0 and g.n_leaves > 0 and nothing()
    assert sim.sdf_stats()["bytes_to_host"] == g.n_leaves * LEAF_BYTES + 4
    # a trails record and an averaged record in the ring: each is taken by its own wait, the other refuses and leaves it outstanding
    assert snap() == 0 and fs.lib.fluid_dist_sdf_snapshot_avg(hd, C.byref(prm), C.byref(avg)) == 0
    assert fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == ERR_STATE and "averaged rank record" in fs.lib.fluid_last_error().decode()
    assert snap() == ERR_STATE                                             # still two
    check_dense(sim.sdf_wait(), *want, n, R, w, dx, "the trails record after a refused wait")
    assert fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == ERR_STATE and fs.lib.fluid_sdf_wait(hd, C.byref(g)) == ERR_STATE
    assert snap() == 0 and snap() == ERR_STATE                             # (one was outstanding: that was the second)
    assert fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == 0 and a.n_leaves > 0
    check_dense(sim.sdf_wait(), *want, n, R, w, dx, "the trails record behind the averaged one")
    assert nothing() and fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == ERR_STATE
    # no instance in the grid: no leaf, NULL pointers, the count alone travels
    hi = sdf_ref.geometry(n)[1]
    sim.upload_particles(np.array([[hi + 2.0, 0.2, -0.3]]), np.array([[-6.0, 0.0, 0.0]]))   # outside, the tail staying out
    assert snap() == 0 and fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == 0
    assert g.n_leaves == 0 and not g.origin and not g.values and not g.active and sim.sdf_stats()["bytes_to_host"] == 4
    assert sim.sdf_dist_trails_stats()["particles"] == 1 and sim.sdf_dist_trails_stats()["instances"] > 1
    sim.close()
    # a handle without a particle
    sim = fs.FluidSim(n=n, dx=dx)
    assert snap_trails(sim, R, w, t).n_leaves == 0 and sim.sdf_dist_trails_stats() == {"particles": 0, "instances": 0}
    sim.close()


def test_record_pointers_survive_moving_cut_planes(fs):
    """The scene of tests/test_gpu_dist_sdf.py's test of this name along 2x1x1: every step is preceded by a record that is waited
    for only after the step; around the step that moves the planes the record's own pinned memory is held against the particles and
    velocities of its moment, before and after the next record is taken from the new window's handle."""
    fd = fs.load_dist()
    n, steps, dims, (R, w, dx) = 32, 8, (2, 1, 1), (1.0, 2.0, 1.0)
    t = (1.0, 1.0, 0.5, 8)
    pos = fs.water_cube_drop(n, 2, seed=0)
    vel = np.random.default_rng(1).standard_normal(pos.shape) * 0.3
    pos = pos + np.array([3.5, 4.5, -2.5])
    solid = np.zeros((n, n, n), dtype=np.uint8)
    solid[:2] = solid[-2:] = 1; solid[:, :2] = solid[:, -2:] = 1; solid[:, :, :2] = solid[:, :, -2:] = 1
    trl = fs.SdfTrails(*t, 0)
    bg = sdf_ref.constants(R, w, dx)[3]

    def work(sim, r):
        sim.set_solid(solid)
        sim.upload_global(pos, vel)
        sim.set_rebalance(4, 1.3)
        moved, checked = [], None
        for k in range(steps):
            before, vbefore, _ = sim.download_local()
            fs.check(fs.lib.fluid_dist_sdf_snapshot_trails(sim._h, C.byref(fs.SdfParams(R, w)), C.byref(trl)))   # outstanding across the step
            st = sim.step()
            moved.append(bool(st["paths"] & REBALANCED))
            gc = fs.SdfGridC()
            fs.check(fs.lib.fluid_dist_sdf_wait(sim._h, C.byref(gc)))
            if not moved[-1] or checked is not None:
                continue
            o, v, m = view(gc)                                             # the handle's own pinned memory, not a copy
            val, act = ref.trails_surface(before, vbefore, n, R, w, dx, t)   # taken from the old window's handle
            wo, wv, wa = sdf_ref.leaf_list(val, act, bg)
            ww = mask_words(wa)
            for what in ("after the step", "after the next record"):
                assert np.array_equal(o, wo) and np.array_equal(u32(v), u32(wv)) and np.array_equal(m, ww), what
                if what == "after the step":
                    now, vnow, _ = sim.download_local()
                    b = snap_trails(sim, R, w, t)                          # the particles as the new window holds them
                    check_trails(b, now, vnow, n, R, w, dx, t)
            checked = dict(k=k, a=fs.SdfGrid(n, o.copy(), v.copy(), wa, gc.background, gc.radius, gc.half_width), b=b, before=before,
                           vbefore=vbefore, now=now, vnow=vnow, stats=sim.sdf_dist_trails_stats(), live=len(now))
        return moved, checked

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dx=dx)
    moved = res[0][0]
    assert any(moved) and all(r[0] == moved for r in res)                  # every rank, in the same steps
    assert all(r[1] is not None and r[1]["k"] == moved.index(True) for r in res)
    assert any(r[1]["a"].n_leaves > 0 for r in res)                        # a non-empty record outlived the swap of the windows
    assert all(r[1]["stats"]["particles"] == r[1]["live"] for r in res)    # the counters went to the new window's handle
    for key, ps, vs in (("a", "before", "vbefore"), ("b", "now", "vnow")):
        check_trails(fs.merge_sdf_grids([r[1][key] for r in res]), np.concatenate([r[1][ps] for r in res]), np.concatenate([r[1][vs] for r in res]),
                     n, R, w, dx, t, key)


def test_dt_is_one_number(fs):
    """What FLUID_BLOCKS_SURFACE_TRAILS=dt rests on: the step all-reduces the maximum speed before it advects, so dt_out is the same
    double on every rank."""
    fd = fs.load_dist()
    n, dims = 24, (2, 2, 1)
    pos = block((3, 3, 3), 2, 9)
    vel = velocities(pos, 10)

    def work(sim, r):
        sim.upload_global(pos, vel)
        return [np.float64(sim.step()["dt_out"]).view(np.uint64) for _ in range(2)]

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dist_solve="decomposed")
    for k in range(2):
        assert len({int(r[k]) for r in res}) == 1, (k, [hex(int(r[k])) for r in res])
        assert np.uint64(res[0][k]).view(np.float64) > 0


@pytest.mark.parametrize("spec", ["dt,0.5", "4,0.5"])
def test_program_on_blocks_writes_the_trails(fs, tmp_path, spec):
    """./run.sh fluid with FLUID_BLOCKS=2x1x1, FLUID_BLOCKS_SURFACE=1.5,2 and FLUID_BLOCKS_SURFACE_TRAILS=dt,0.5 at n = 24, 2 steps
    (free fall from rest: at shutter = dt every particle is still one instance), and with SHUTTER = 4, where the fall makes more:
    surface<i>.vdb holds the reference's grid, and exactly its leaves, of the blocks' own particles, velocities and dt_out of step i
    (the same run repeated here with the program's cut planes and upload).  Stdout and the density files are what they are without
    the two variables.  Whether the file also equals the one-GPU FLUID_OUT_SURFACE_TRAILS file is printed, not asserted."""
    fd = fs.load_dist()
    n, ppc, steps, blocks, (R, w, dx) = 24, 2, 2, "2x1x1", (1.5, 2.0, 1.0)
    lo, hi, _, _ = sdf_ref.geometry(n)
    outs = {}
    for mode in ("plain", "trails", "one"):
        d = tmp_path / mode
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k not in MORE_VARS}
        env.update(FLUID_N=str(n), FLUID_PPC=str(ppc), FLUID_STEPS=str(steps), FLUID_OUT=str(d / "simulation"))
        if mode == "one":
            env.update(FLUID_OUT_SURFACE=f"{R},{w}", FLUID_OUT_SURFACE_TRAILS=spec)
        else:
            env.update(FLUID_BLOCKS=blocks)
        if mode == "trails":
            env.update(FLUID_BLOCKS_SURFACE=f"{R},{w}", FLUID_BLOCKS_SURFACE_TRAILS=spec)
        r = subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=d, timeout=600)
        assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["plain"] == outs["trails"]
    assert not list((tmp_path / "plain").rglob("surface*"))
    for nm in ["mygrids.vdb"] + [f"simulation/mygrids{i}.vdb" for i in range(steps)]:
        assert leaf_ref.same_file(tmp_path / "plain" / nm, tmp_path / "trails" / nm), nm
    dims = tuple(int(x) for x in blocks.split("x"))
    pos = fs.water_cube_drop(n, ppc, seed=0)

    def work(sim, r):
        sim.upload_global(pos)
        out = []
        for _ in range(steps):
            st = sim.step()
            p, v, _ = sim.download_local()
            out.append((p, v, st["dt_out"]))
        return out

    res = run_group(fs, dims, n, fd.partition_blocks(n, pos, dims), work)
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        dt = res[0][i][2]
        assert all(r[i][2] == dt for r in res)
        t = (dt if spec.startswith("dt") else 4.0, 0.5, R / 2, 16)         # DELTA 0.5, RMIN defaults to R / 2, MAX to 16
        p, v = np.concatenate([r[i][0] for r in res]), np.concatenate([r[i][1] for r in res])
        P, rad, _ = ref.instances(p, v, R, t)
        val, act = ref.union(P, rad, n, R, w, dx)
        _, grids = vdb_reader.read(tmp_path / "trails" / f"simulation/surface{i}.vdb")
        assert len(grids) == 1 and grids[0].name == "surface" and grids[0].metadata["class"] == "level set"
        assert np.float32(grids[0].background) == bg
        rv, ra = grids[0].dense(lo, hi)
        assert act.any() and np.array_equal(u32(rv), u32(val)) and np.array_equal(ra, act), i
        assert sorted(grids[0].leaves) == [tuple(o) for o in sdf_ref.leaf_list(val, act, bg)[0].tolist()]
        same = leaf_ref.same_file(tmp_path / "one" / f"simulation/surface{i}.vdb", tmp_path / "trails" / f"simulation/surface{i}.vdb")
        print(f"step {i}: dt {dt!r} particles {len(p)} instances {len(P)} equals the one-GPU file: {same}")
    if not spec.startswith("dt"):
        assert len(P) > len(p)                                             # the last step's surface is not the spheres'
