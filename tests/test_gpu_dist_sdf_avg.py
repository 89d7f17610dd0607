"""GPU (-m gpu): the averaged-position surface of a decomposed run (include/fluid_hip.h, "liquid surface, averaged positions
(decomposed runs)"): the rank records of fluid_dist_sdf_snapshot_avg / _wait_avg (k_sdf_search_avg<true>, k_sdf_pack_avg) against
tests/sdf_avg_part_ref.py record() of the rank's downloaded live positions, and their merge (fluid_sdf_avg_grids_merge) against the
one-GPU AVERAGED snapshot of all downloaded positions and against sdf_avg_ref.averaged() of them.  Every comparison is exact: bit
patterns of dist2 and values, equality of sums, masks and origins.  Blocks run as threads of a LocalGroup on the one GPU of the box;
the helpers follow tests/test_gpu_dist_sdf.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import leaf_ref
import sdf_avg_part_ref as part_ref
import sdf_avg_ref
import sdf_ref
import vdb_reader
from sdf_testlib import FLUID, FLUID_VARS, same_grid, u32

pytestmark = pytest.mark.gpu

PARAMS = [(1.5, 2.5, 1.0, 4.0), (1.0, 1.0, 1.0, 4.0)]      # (R, w, dx, h); the second: hf > R + w, records reach beyond the band
LEAF_BYTES = 2048 + 64 + 12                               # FLUID_SDF_LEAF_BYTES
ERR_ARG, ERR_STATE = 1, 3
REBALANCED = 32                                           # FLUID_PATH_DIST_REBALANCED
CASES = [                                                 # those of tests/test_gpu_dist_sdf.py
    (16, (2, 1, 1), (3, 3, 3)),
    (25, (2, 2, 1), (3, 3, 3)),          # odd N: the first leaf starts outside the grid
    (32, (2, 2, 2), (3, 3, 3)),          # the leaf around the corner of the eight blocks
    (24, (1, 1, 3), (2, 2, 6)),          # a middle block with a cut on either side
]


def block(h, ppc, seed, centre=(0, 0, 0)):
    """`ppc` points in every cell of [c - h, c + h) per axis."""
    rng = np.random.default_rng(seed)
    ax = [np.arange(centre[a] - h[a], centre[a] + h[a]) for a in range(3)]
    c = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.repeat(c, ppc, axis=0) + rng.uniform(-0.49, 0.49, (ppc * len(c), 3))


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


def snap_avg(sim, R, w, h):
    sim.sdf_snapshot_avg(R, w, h)
    return sim.sdf_wait_avg()


def entries(fs, sim):
    """Entries of the handle's particle arrays, the dead ones included."""
    return int(fs.lib.fluid_num_particles(sim._h))


def check_record(a, pos, n, R, w, dx, h, what=""):
    """a is exactly the canonical rank record of the particles `pos`."""
    org, d2, sums = part_ref.record(pos, n, R, w, dx, h)
    fR, fw, dxf, bg, _, _ = sdf_ref.constants(R, w, dx)
    assert a.n == n and (a.background, a.radius, a.half_width, a.dx, a.influence) == (bg, fR, fw, dxf, np.float32(h)), what
    assert a.n_leaves == len(org), (what, a.n_leaves, len(org))
    assert np.array_equal(a.origin, org), what
    assert np.array_equal(u32(a.dist2), u32(d2)), what
    assert np.array_equal(a.sums, sums), what


def check_avg(g, pos, n, R, w, dx, h, what=""):
    """g is exactly the leaf list of the reference's averaged grid for the particles `pos`."""
    val, act = sdf_avg_ref.averaged(pos, n, R, w, dx, h)
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert g.n == n and (g.background, g.radius, g.half_width) == (bg, fR, fw), what
    assert g.n_leaves == len(org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.origin, org) and np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what
    return val, act


def one_gpu(fs, pos, n, R, w, dx, h):
    """fluid_sdf_snapshot under AVERAGED on one handle that holds `pos`."""
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    sim.sdf_set_surface("averaged", h)
    sim.sdf_snapshot(R, w)
    g = sim.sdf_wait()
    sim.close()
    return g


@pytest.mark.parametrize("R,w,dx,h", PARAMS)
@pytest.mark.parametrize("n,dims,hb", CASES, ids=[f"n{c[0]}" for c in CASES])
def test_rank_records_and_their_merge(fs, n, dims, hb, R, w, dx, h):
    fd = fs.load_dist()
    pos = block(hb, 2, n)
    _, _, _, nl = sdf_ref.geometry(n)

    def work(sim, r):
        sim.upload_global(pos)
        out = []
        for k in range(4):
            if k:
                sim.step()
            a = snap_avg(sim, R, w, h)
            p, _, _ = sim.download_local()
            check_record(a, p, n, R, w, dx, h, (r, k))
            st = sim.sdf_stats()
            assert st == {"leaves_in_grid": nl ** 3, "leaves_listed": a.n_leaves, "bytes_to_host": a.n_leaves * part_ref.LEAF_BYTES + 4}
            out.append(dict(a=a, p=p, dead=entries(fs, sim) - len(p)))
        return out

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dist_solve="decomposed")
    assert all(len(r[0]["p"]) > 0 for r in res)                            # the block straddles the cuts: every rank holds some
    for k in range(4):
        parts = [r[k]["a"] for r in res]
        allp = np.concatenate([r[k]["p"] for r in res])
        merged = fs.merge_sdf_avg_grids(parts)
        check_avg(merged, allp, n, R, w, dx, h, k)
        same_grid(merged, one_gpu(fs, allp, n, R, w, dx, h), f"one GPU, snapshot {k}")
        assert sum(p.n_leaves for p in parts) > merged.n_leaves > 0          # a leaf near a cut is listed from both sides
        dead = [r[k]["dead"] for r in res]
        print(f"snapshot {k}: record leaves per rank {[p.n_leaves for p in parts]} merged {merged.n_leaves} dead entries {dead}")
        assert all(d == 0 for d in dead) if k == 0 else max(dead) > 0        # after a step the served ghosts are still in the arrays


def test_two_particles_across_the_cut(fs):
    """The list rule's scene: rank B weighs on voxels of A's band in leaves its own spheres' list does not hold."""
    fd = fs.load_dist()
    n, (R, w, dx, h), A, B = part_ref.two_particles()
    pos, dims = np.vstack([A, B]), (2, 1, 1)

    def work(sim, r):
        sim.upload_global(pos)
        p, _, _ = sim.download_local()
        a = snap_avg(sim, R, w, h)
        check_record(a, p, n, R, w, dx, h, r)
        sim.sdf_snapshot(R, w)
        return a, sim.sdf_wait(), p

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work)
    assert np.array_equal(res[0][2], A) and np.array_equal(res[1][2], B)     # the cut separates them
    rec = {tuple(o) for o in res[1][0].origin.tolist()}
    sph = {tuple(o) for o in res[1][1].origin.tolist()}
    assert len(rec) == 8 and len(sph) == 4 and sph < rec
    merged = fs.merge_sdf_avg_grids([r[0] for r in res])
    check_avg(merged, pos, n, R, w, dx, h)
    same_grid(merged, one_gpu(fs, pos, n, R, w, dx, h), "one GPU")


def test_interior_and_early_stop(fs):
    """A filled 8^3 block with 8 points per cell astride the cut, (R, w) = (3, 1), one cell from the grid's corner in y and z: the
    voxels with m <= min2 carry +0 and no sums, also in the x planes whose in-grid voxels are all that deep (the search stops those
    planes early and leaves m and the sums unfinished), and the merge is exact."""
    fd = fs.load_dist()
    n, dims, (R, w, dx, h) = 24, (2, 1, 1), (3.0, 1.0, 1.0, 4.0)
    pos = block((4, 4, 4), 8, 7, centre=(0, -7, -7))
    min2 = sdf_ref.constants(R, w, dx)[5]

    def work(sim, r):
        sim.upload_global(pos)
        p, _, _ = sim.download_local()
        a = snap_avg(sim, R, w, h)
        check_record(a, p, n, R, w, dx, h, r)
        return a, p

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work)
    for a, p in res:
        m = part_ref.to_leaves(sdf_avg_ref.sums(p, n, h)[0], n, np.float32(np.inf))
        _, _, l0, nl = sdf_ref.geometry(n)
        c = (a.origin.astype(np.int64) - l0) // 8
        j = (c[:, 0] * nl + c[:, 1]) * nl + c[:, 2]
        deep = m[j] <= min2
        ingrid = part_ref.to_leaves(np.ones((n, n, n), bool), n, False)[j]
        planes = ((deep | ~ingrid).reshape(-1, 8, 64).all(axis=2) & ingrid.reshape(-1, 8, 64).any(axis=2))
        assert deep.sum() > 100 and planes.any()                             # some x plane of a listed leaf stops early
        assert (u32(a.dist2[deep]) == 0).all() and not a.sums[np.broadcast_to(deep[:, None, :], a.sums.shape)].any()
    allp = np.concatenate([r[1] for r in res])
    merged = fs.merge_sdf_avg_grids([r[0] for r in res])
    val, act = check_avg(merged, allp, n, R, w, dx, h)
    assert (val[~act] < 0).any()                                             # the inactive -bg interior
    same_grid(merged, one_gpu(fs, allp, n, R, w, dx, h), "one GPU")


def test_removed_particles_do_not_count(fs):
    fd = fs.load_dist()
    n, dims, (R, w, dx, h) = 24, (2, 1, 1), PARAMS[0]
    pos = block((4, 3, 3), 2, 5)
    lo, hi = (9, 9, 9), (13, 14, 14)                                       # array indices: part of the block, across the cut at 12

    def work(sim, r):
        sim.upload_global(pos)
        sim.set_sink(0, lo, hi)
        sim.step()
        a = snap_avg(sim, R, w, h)
        p, _, _ = sim.download_local()
        check_record(a, p, n, R, w, dx, h, r)
        return dict(a=a, p=p, dead=entries(fs, sim) - len(p), removed=sim.source_stats()["removed_last"])

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dist_solve="decomposed")
    p = np.concatenate([r["p"] for r in res])
    assert res[0]["removed"] > 0 and len(p) == len(pos) - res[0]["removed"]
    assert all(r["dead"] > 0 for r in res)                                 # the removed particles (and ghosts) are still in the arrays
    check_avg(fs.merge_sdf_avg_grids([r["a"] for r in res]), p, n, R, w, dx, h)


@pytest.mark.parametrize("n", [16, 25])
def test_plain_handle(fs, n):
    """The record of a plain FluidSim merged alone is its own AVERAGED snapshot."""
    R, w, dx, h = PARAMS[0]
    pos = block((3, 3, 3), 2, n)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    sim.step()
    p = sim.download_particles()[0]
    a = snap_avg(sim, R, w, h)
    check_record(a, p, n, R, w, dx, h)
    merged = fs.merge_sdf_avg_grids([a])
    check_avg(merged, p, n, R, w, dx, h)
    sim.sdf_set_surface("averaged", h)
    sim.sdf_snapshot(R, w)
    same_grid(merged, sim.sdf_wait(), "the handle's own AVERAGED snapshot")
    sim.close()


def test_slots_kinds_and_refusals(fs):
    n, (R, w, dx, h) = 16, PARAMS[0]
    pos = block((3, 3, 3), 2, 3)
    sim = fs.FluidSim(n=n)
    hd = sim._h
    sim.upload_particles(pos)
    prm, avg = fs.SdfParams(R, w), fs.SdfSurface(1, 0, h)
    g, a, at, ap = fs.SdfGridC(), fs.SdfAvgPartC(), fs.SdfAttrC(), fs.SdfAttrPartC()
    snap = lambda: fs.lib.fluid_dist_sdf_snapshot_avg(hd, C.byref(prm), C.byref(avg))   # noqa: E731
    # bad arguments: refused, nothing outstanding
    assert fs.lib.fluid_dist_sdf_snapshot_avg(None, C.byref(prm), C.byref(avg)) == ERR_ARG
    assert fs.lib.fluid_dist_sdf_snapshot_avg(hd, None, C.byref(avg)) == ERR_ARG
    assert fs.lib.fluid_dist_sdf_snapshot_avg(hd, C.byref(prm), None) == ERR_ARG
    for kind, res, infl in ((0, 0, 3.0), (2, 0, 3.0), (-1, 0, 3.0), (1, 1, 3.0), (1, 0, 0.0), (1, 0, -1.0), (1, 0, 4.5), (1, 0, float("nan"))):
        assert fs.lib.fluid_dist_sdf_snapshot_avg(hd, C.byref(prm), C.byref(fs.SdfSurface(kind, res, infl))) == ERR_ARG, (kind, res, infl)
    for bad in ((2.0, 2.5), (1.5, 0.5), (0.0, 2.0), (float("nan"), 2.0)):
        assert fs.lib.fluid_dist_sdf_snapshot_avg(hd, C.byref(fs.SdfParams(*bad)), C.byref(avg)) == ERR_ARG, bad
    assert fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == ERR_STATE and fs.lib.fluid_dist_sdf_wait_avg(hd, None) == ERR_ARG
    assert fs.lib.fluid_dist_sdf_wait_avg(None, C.byref(a)) == ERR_ARG
    # the handle's own setting is neither read nor changed: a spheres snapshot is byte for byte what it was
    sim.sdf_snapshot(R, w)
    before = sim.sdf_wait()
    assert snap() == 0 and fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == 0 and a.n_leaves > 0
    sim.sdf_snapshot(R, w)
    after = sim.sdf_wait()
    same_grid(after, before, "spheres after a record")
    assert after.values.tobytes() == before.values.tobytes()
    assert sim.sdf_stats()["bytes_to_host"] == after.n_leaves * LEAF_BYTES + 4
    # two outstanding snapshots of mixed kinds; a third is refused
    sim.sdf_snapshot(R, w)
    assert snap() == 0
    assert snap() == ERR_STATE and "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_snapshot(hd, C.byref(prm)) == ERR_STATE
    # the oldest is a spheres list: the record's wait refuses and leaves it outstanding
    assert fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == ERR_STATE and "averaged rank record" in fs.lib.fluid_last_error().decode()
    assert snap() == ERR_STATE                                             # still two
    same_grid(sim.sdf_wait(), before, "the list after a refused wait")
    # now the oldest is a record: the four other waits refuse and leave it outstanding
    assert fs.lib.fluid_sdf_wait(hd, C.byref(g)) == ERR_STATE and "fluid_dist_sdf_wait_avg" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == ERR_STATE
    assert fs.lib.fluid_sdf_wait_attr(hd, C.byref(g), C.byref(at)) == ERR_STATE
    assert fs.lib.fluid_dist_sdf_wait_attr(hd, C.byref(g), C.byref(ap)) == ERR_STATE
    sim.sdf_snapshot(R, w)                                                 # (one was outstanding: this is the second)
    assert snap() == ERR_STATE
    rec = sim.sdf_wait_avg()
    check_record(rec, pos, n, R, w, dx, h)
    same_grid(sim.sdf_wait(), before, "the list behind the record")
    assert fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == ERR_STATE and fs.lib.fluid_sdf_wait(hd, C.byref(g)) == ERR_STATE   # nothing outstanding
    # under the handle's AVERAGED setting the record is the same, and the setting stays
    sim.sdf_set_surface("averaged", 2.0)
    rec2 = snap_avg(sim, R, w, h)
    assert np.array_equal(rec2.origin, rec.origin) and rec2.dist2.tobytes() == rec.dist2.tobytes() and np.array_equal(rec2.sums, rec.sums)
    sim.sdf_snapshot(R, w)
    check_avg(sim.sdf_wait(), pos, n, R, w, dx, 2.0, "the setting's own influence")
    # no particle: no leaf, NULL pointers, the count alone travels
    sim.upload_particles(np.array([[sdf_ref.geometry(n)[1] + 0.6, 0.0, 0.0]]))   # base cell outside the grid: it does not count
    assert snap() == 0 and fs.lib.fluid_dist_sdf_wait_avg(hd, C.byref(a)) == 0
    assert a.n_leaves == 0 and not a.origin and not a.dist2 and not a.sums and sim.sdf_stats()["bytes_to_host"] == 4
    sim.close()


def test_record_pointers_survive_moving_cut_planes(fs):
    """The scene of tests/test_gpu_dist_sdf.py's test of this name along 2x1x1: every step is preceded by a record that is waited
    for only after the step; around the step that moves the planes the record's own pinned memory is held against the particles of
    its moment, before and after the next record is taken from the new window's handle."""
    fd = fs.load_dist()
    n, steps, dims, (R, w, dx, h) = 32, 8, (2, 1, 1), (1.0, 1.0, 1.0, 3.0)
    pos = fs.water_cube_drop(n, 2, seed=0)
    vel = np.random.default_rng(1).standard_normal(pos.shape) * 0.3
    pos = pos + np.array([3.5, 4.5, -2.5])
    solid = np.zeros((n, n, n), dtype=np.uint8)
    solid[:2] = solid[-2:] = 1; solid[:, :2] = solid[:, -2:] = 1; solid[:, :, :2] = solid[:, :, -2:] = 1
    avg = fs.SdfSurface(1, 0, h)

    def view(ac):
        k = ac.n_leaves
        if k == 0:
            return np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 4, 512), np.uint64)
        o = np.ctypeslib.as_array(C.cast(ac.origin, C.POINTER(C.c_int32)), shape=(k, 3))
        d = np.ctypeslib.as_array(C.cast(ac.dist2, C.POINTER(C.c_float)), shape=(k, 512))
        s = np.ctypeslib.as_array(C.cast(ac.sums, C.POINTER(C.c_uint64)), shape=(k, 4, 512))
        return o, d, s

    def work(sim, r):
        sim.set_solid(solid)
        sim.upload_global(pos, vel)
        sim.set_rebalance(4, 1.3)
        moved, checked = [], None
        for k in range(steps):
            before, _, _ = sim.download_local()
            fs.check(fs.lib.fluid_dist_sdf_snapshot_avg(sim._h, C.byref(fs.SdfParams(R, w)), C.byref(avg)))   # outstanding across the step
            st = sim.step()
            moved.append(bool(st["paths"] & REBALANCED))
            ac = fs.SdfAvgPartC()
            fs.check(fs.lib.fluid_dist_sdf_wait_avg(sim._h, C.byref(ac)))
            if not moved[-1] or checked is not None:
                continue
            o, d, s = view(ac)                                             # the handle's own pinned memory, not a copy
            want = part_ref.record(before, n, R, w, dx, h)                 # taken from the old window's handle
            for what in ("after the step", "after the next record"):
                assert np.array_equal(o, want[0]) and np.array_equal(u32(d), u32(want[1])) and np.array_equal(s, want[2]), what
                if what == "after the step":
                    now, _, _ = sim.download_local()
                    b = snap_avg(sim, R, w, h)                             # the particles as the new window holds them
                    check_record(b, now, n, R, w, dx, h)
            checked = dict(k=k, a=fs.SdfAvgPart(ac.n, o.copy(), d.copy(), s.copy(), ac.background, ac.radius, ac.half_width, ac.dx, ac.influence),
                           b=b, before=before, now=now)
        return moved, checked

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), work, dx=dx)
    moved = res[0][0]
    assert any(moved) and all(r[0] == moved for r in res)                  # every rank, in the same steps
    assert all(r[1] is not None and r[1]["k"] == moved.index(True) for r in res)
    assert any(r[1]["a"].n_leaves > 0 for r in res)                        # a non-empty record outlived the swap of the windows
    for key, ps in (("a", "before"), ("b", "now")):
        check_avg(fs.merge_sdf_avg_grids([r[1][key] for r in res]), np.concatenate([r[1][ps] for r in res]), n, R, w, dx, h)


def test_program_on_blocks_writes_the_averaged_surface(fs, tmp_path):
    """./run.sh fluid with FLUID_BLOCKS=2x1x1, FLUID_BLOCKS_SURFACE=1,3 and FLUID_BLOCKS_SURFACE_KIND=averaged,3 at n = 24, 2 steps (the
    smallest grid the program cuts in two: fluid_partition_blocks wants n >= 8 P + 8 along an axis of P blocks, so n = 16 is refused).
    At this size the block run's particles agree bit for bit with the one-GPU run's (measured on an MI355X: both surface files
    equal), so surface<i>.vdb must equal, outside the uuid, the file the one-GPU run writes with FLUID_OUT_SURFACE_KIND=averaged,3; it
    is also held to the reference's averaged grid of the blocks' own particles of step i (the same run repeated here with the
    program's cut planes and upload).  Stdout and the density files are what they are without the two variables."""
    fd = fs.load_dist()
    n, ppc, steps, blocks, (R, w, dx, h) = 24, 2, 2, "2x1x1", (1.0, 3.0, 1.0, 3.0)
    lo, hi, _, _ = sdf_ref.geometry(n)
    outs = {}
    for mode in ("plain", "averaged", "one"):
        d = tmp_path / mode
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k not in ("FLUID_OUT_SURFACE_KIND", "FLUID_BLOCKS_SURFACE_KIND")}
        env.update(FLUID_N=str(n), FLUID_PPC=str(ppc), FLUID_STEPS=str(steps), FLUID_OUT=str(d / "simulation"))
        if mode == "one":
            env.update(FLUID_OUT_SURFACE=f"{R},{w}", FLUID_OUT_SURFACE_KIND=f"averaged,{h}")
        else:
            env.update(FLUID_BLOCKS=blocks)
        if mode == "averaged":
            env.update(FLUID_BLOCKS_SURFACE=f"{R},{w}", FLUID_BLOCKS_SURFACE_KIND=f"averaged,{h}")
        r = subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=d, timeout=600)
        assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["plain"] == outs["averaged"]
    assert not list((tmp_path / "plain").rglob("surface*"))
    for nm in ["mygrids.vdb"] + [f"simulation/mygrids{i}.vdb" for i in range(steps)]:
        assert leaf_ref.same_file(tmp_path / "plain" / nm, tmp_path / "averaged" / nm), nm
    dims = tuple(int(x) for x in blocks.split("x"))
    pos = fs.water_cube_drop(n, ppc, seed=0)

    def work(sim, r):
        sim.upload_global(pos)
        out = []
        for _ in range(steps):
            sim.step()
            out.append(sim.download_local()[0])
        return out

    res = run_group(fs, dims, n, fd.partition_blocks(n, pos, dims), work)
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        val, act = sdf_avg_ref.averaged(np.concatenate([r[i] for r in res]), n, R, w, dx, h)
        _, grids = vdb_reader.read(tmp_path / "averaged" / f"simulation/surface{i}.vdb")
        assert len(grids) == 1 and grids[0].name == "surface" and grids[0].metadata["class"] == "level set"
        assert np.float32(grids[0].background) == bg
        rv, ra = grids[0].dense(lo, hi)
        assert act.any() and np.array_equal(u32(rv), u32(val)) and np.array_equal(ra, act), i
        assert sorted(grids[0].leaves) == [tuple(o) for o in sdf_ref.leaf_list(val, act, bg)[0].tolist()]
        same = leaf_ref.same_file(tmp_path / "one" / f"simulation/surface{i}.vdb", tmp_path / "averaged" / f"simulation/surface{i}.vdb")
        assert same, i
