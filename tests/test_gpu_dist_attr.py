"""GPU (-m gpu): surface attributes of a decomposed run (include/fluid_hip.h, "liquid surface, attributes (decomposed runs)"):
the rank records of fluid_dist_sdf_snapshot_attr / fluid_dist_sdf_wait_attr (the third mode of k_sdf_search and k_sdf_pack) and
their merge, fluid_sdf_attr_grids_merge.  Blocks run as threads of a LocalGroup on the one GPU of the box, as in
tests/test_gpu_dist_sdf.py, whose scenes these are.  The reference of every record is tests/attr_merge_ref.py on the particles
downloaded from the handles — a rank's own for its record, all ranks' together for the merge; everything is compared with ==."""
import ctypes as C

import numpy as np
import pytest

import attr_merge_ref
import attr_ref
import leaf_ref
import mesh_ref
import sdf_filter_ref
import sdf_ref
from test_gpu_attr import read_ply
from test_gpu_dist_sdf import CASES, MODES, REBALANCED, SETS, block, entries, run_fluid, run_group, u32, view

pytestmark = pytest.mark.gpu

LEAF_BYTES = 2048 + 64 + 12                               # FLUID_SDF_LEAF_BYTES
PART_BYTES = 2048 + 6144 + 2048                           # FLUID_SDF_ATTR_PART_LEAF_BYTES
ERR_ARG, ERR_STATE = 1, 3
NO_ID = 0xFFFFFFFF


def snap(sim, R, w):
    sim.sdf_snapshot(R, w, attr=True)
    return sim.sdf_wait_attr()


def check_record(g, a, pos, vel, ids, n, R, w, dx):
    """(g, a) is exactly the rank record of the particles (pos, vel, ids)."""
    ref = attr_merge_ref.rank_record(pos, vel, ids, n, R, w, dx)
    assert g.n_leaves == a.n_leaves == len(ref["origin"]), (g.n_leaves, a.n_leaves, len(ref["origin"]))
    assert np.array_equal(g.origin, ref["origin"]) and np.array_equal(g.active, ref["active"])
    assert np.array_equal(u32(g.values), u32(ref["values"]))
    assert np.array_equal(a.id, ref["id"])
    assert np.array_equal(u32(a.velocity), u32(ref["velocity"]))
    assert np.array_equal(u32(a.dist2), u32(ref["dist2"]))
    assert ((a.id == NO_ID) == ~g.active).all() and (u32(a.dist2)[~g.active] == 0x7F800000).all()
    assert np.isin(a.id[g.active], ids).all()                              # no id the rank does not hold alive (never PID_DEAD)


def check_merged(fs, res_g, res_a, pos, vel, ids, n, R, w, dx):
    grid, attr = fs.merge_sdf_attr_grids(res_g, res_a)
    ref = attr_merge_ref.merged(pos, vel, ids, n, R, w, dx)
    assert np.array_equal(grid.origin, ref["origin"]) and np.array_equal(grid.active, ref["active"])
    assert np.array_equal(u32(grid.values), u32(ref["values"]))
    assert np.array_equal(attr.id, ref["id"]) and np.array_equal(u32(attr.velocity), u32(ref["velocity"]))
    plain = fs.merge_sdf_grids(res_g)
    assert plain.origin.tobytes() == grid.origin.tobytes() and plain.values.tobytes() == grid.values.tobytes()
    assert np.array_equal(plain.active, grid.active)
    return grid, attr


def same_geometry(a, b):
    return a.origin.tobytes() == b.origin.tobytes() and a.values.tobytes() == b.values.tobytes() and np.array_equal(a.active, b.active)


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,dims,h", CASES, ids=[f"n{c[0]}" for c in CASES])
def test_rank_records_and_their_merge(fs, mode, n, dims, h, R, w, dx):
    fd = fs.load_dist()
    pos = block(h, 2, n)
    vel = attr_ref.velocities(pos) * 0.1
    _, _, _, nl = sdf_ref.geometry(n)

    def work(sim, r):
        sim.upload_global(pos, vel)
        out = []
        for k in range(4):
            if k:
                sim.step()
            if k in (1, 2):
                continue
            g, a = snap(sim, R, w)
            p, v, ids = sim.download_local()                               # after steps: sort order, not id order
            check_record(g, a, p, v, ids, n, R, w, dx)
            st = sim.sdf_stats()
            assert st == {"leaves_in_grid": nl ** 3, "leaves_listed": g.n_leaves, "bytes_to_host": g.n_leaves * (LEAF_BYTES + PART_BYTES) + 4}
            sim.sdf_snapshot(R, w)                                         # the plain snapshot of the same state: the same bytes
            assert same_geometry(sim.sdf_wait(), g)
            out.append(dict(g=g, a=a, p=p, v=v, ids=ids, dead=entries(fs, sim) - len(p)))
        return out

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), mode, work)
    assert all(len(r[0]["p"]) > 0 for r in res)
    for k in range(2):
        cat = lambda key: np.concatenate([r[k][key] for r in res])         # noqa: E731
        ids = cat("ids")
        assert len(np.unique(ids)) == len(ids) == len(pos)
        grid, attr = check_merged(fs, [r[k]["g"] for r in res], [r[k]["a"] for r in res], cat("p"), cat("v"), ids, n, R, w, dx)
        assert sum(r[k]["g"].n_leaves for r in res) > grid.n_leaves > 0
        assert np.isin(attr.id[grid.active], ids).all()
        dead = [r[k]["dead"] for r in res]
        assert all(d == 0 for d in dead) if k == 0 else max(dead) > 0      # after steps the served ghosts are still in the arrays
        if k:
            assert any((np.diff(r[k]["ids"].astype(np.int64)) < 0).any() for r in res)      # ... and the arrays are not in id order


BUILT = {"near": (np.array([[-2.75 - 2e-7, 0.1, 0.2], [2.75, 0.1, 0.2]]), 13, 1),        # positions, voxels to find, id they must get
         "tie": (np.array([[2.75, 0.1, 0.2], [-2.75, 0.1, 0.2]]), 24, 0)}                  # rank 1 holds id 0
BUILT_VEL = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.125]])


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("scene", ["near", "tie"])
def test_the_two_built_cases(fs, scene, R, w, dx):
    """One particle on either side of the cut at x = 0.  near: both ranks hold 13 voxels active with bit-equal values, and the
    right particle (id 1, the later part) is strictly closer.  tie: 24 voxels tie on dist2 itself, and the later part holds id 0."""
    fd = fs.load_dist()
    n, dims = 16, (2, 1, 1)
    pos, want, winner = BUILT[scene]

    def work(sim, r):
        sim.upload_global(pos, BUILT_VEL)
        g, a = snap(sim, R, w)
        p, v, ids = sim.download_local()
        check_record(g, a, p, v, ids, n, R, w, dx)
        return g, a, p, v, ids

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), "decomposed", work)
    assert [len(r[2]) for r in res] == [1, 1] and res[0][2][0, 0] < 0 < res[1][2][0, 0]
    assert res[1][4][0] == (1 if scene == "near" else 0)
    grid, attr = check_merged(fs, [r[0] for r in res], [r[1] for r in res], pos, BUILT_VEL, np.arange(2, dtype=np.uint32), n, R, w, dx)
    (g0, a0), (g1, a1) = res[0][:2], res[1][:2]
    at0 = {tuple(o): k for k, o in enumerate(g0.origin.tolist())}
    atm = {tuple(o): k for k, o in enumerate(grid.origin.tolist())}
    count = 0
    for k1, o in enumerate(map(tuple, g1.origin.tolist())):
        if o not in at0:
            continue
        k0 = at0[o]
        both = g0.active[k0] & g1.active[k1]
        if scene == "near":
            hit = both & (u32(g0.values[k0]) == u32(g1.values[k1])) & (a0.dist2[k0] != a1.dist2[k1])
            assert (a1.dist2[k1][hit] < a0.dist2[k0][hit]).all()
        else:
            hit = both & (a0.dist2[k0] == a1.dist2[k1])
        count += int(hit.sum())
        assert (attr.id[atm[o]][hit] == winner).all()
    print(f"{scene} R={R} w={w}: {count} voxels")
    assert count == want


def test_one_handle_with_the_same_ids_and_a_plain_handle(fs):
    fd = fs.load_dist()
    n, dims, h = CASES[1]
    R, w, dx = SETS[0]
    pos = block(h, 2, n)
    vel = attr_ref.velocities(pos) * 0.1

    def work(sim, r):
        sim.upload_global(pos, vel)
        sim.step()
        return snap(sim, R, w) + tuple(sim.download_local())

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), "decomposed", work)
    p, v, ids = (np.concatenate([r[k] for r in res]) for k in (2, 3, 4))
    grid, attr = fs.merge_sdf_attr_grids([r[0] for r in res], [r[1] for r in res])
    one = fs.FluidSim(n=n)
    one.upload_particles_ids(p, v, ids)
    one.sdf_snapshot(R, w, attr=True)
    g1, a1 = one.sdf_wait_attr()
    assert same_geometry(g1, grid) and grid.n_leaves > 0
    assert np.array_equal(a1.id, attr.id) and np.array_equal(u32(a1.velocity), u32(attr.velocity))
    # the decomposed entry points on this plain handle: the one-GPU attributes, and dist2
    h_ = one._h
    gc, pc = fs.SdfGridC(), fs.SdfAttrPartC()
    fs.check(fs.lib.fluid_dist_sdf_snapshot_attr(h_, C.byref(fs.SdfParams(R, w))))
    fs.check(fs.lib.fluid_dist_sdf_wait_attr(h_, C.byref(gc), C.byref(pc)))
    g2, a2 = view(fs, gc), view_part(pc)
    assert same_geometry(g2, g1) and np.array_equal(a2.id, a1.id) and np.array_equal(u32(a2.velocity), u32(a1.velocity))
    check_record(g2, a2, p, v, ids, n, R, w, dx)
    st = one.sdf_stats()
    assert st["bytes_to_host"] == g2.n_leaves * (LEAF_BYTES + PART_BYTES) + 4
    one.close()
    # uploaded without ids: the ids are rows of fluid_download_particles
    two = fs.FluidSim(n=n)
    two.upload_particles(p, v)
    two.step()
    fs.check(fs.lib.fluid_dist_sdf_snapshot_attr(two._h, C.byref(fs.SdfParams(R, w))))
    fs.check(fs.lib.fluid_dist_sdf_wait_attr(two._h, C.byref(gc), C.byref(pc)))
    g3, a3 = view(fs, gc), view_part(pc)
    dp, dv = two.download_particles()[:2]
    check_record(g3, a3, dp, dv, np.arange(len(dp), dtype=np.uint32), n, R, w, dx)
    two.sdf_snapshot(R, w, attr=True)
    g4, a4 = two.sdf_wait_attr()
    assert same_geometry(g3, g4) and np.array_equal(a3.id, a4.id) and np.array_equal(u32(a3.velocity), u32(a4.velocity))
    two.close()


class Part:
    pass


def view_part(pc):
    """The record over the handle's own pinned memory (no copy)."""
    k = pc.n_leaves
    a = Part()
    a.n_leaves = k
    if k == 0 or not pc.id:
        assert not pc.id and not pc.velocity and not pc.dist2
        a.id = a.velocity = a.dist2 = None
        return a
    a.id = np.ctypeslib.as_array(C.cast(pc.id, C.POINTER(C.c_uint32)), shape=(k, 512))
    a.velocity = np.ctypeslib.as_array(C.cast(pc.velocity, C.POINTER(C.c_float)), shape=(k, 3, 512))
    a.dist2 = np.ctypeslib.as_array(C.cast(pc.dist2, C.POINTER(C.c_float)), shape=(k, 512))
    return a


def test_removed_particles_do_not_count(fs):
    fd = fs.load_dist()
    n, dims, (R, w, dx) = 24, (2, 1, 1), SETS[0]
    pos = block((4, 3, 3), 2, 5)
    vel = attr_ref.velocities(pos) * 0.1
    lo, hi = (9, 9, 9), (13, 14, 14)                                       # array indices: part of the block, across the cut at 12

    def work(sim, r):
        sim.upload_global(pos, vel)
        sim.set_sink(0, lo, hi)
        sim.step()
        g, a = snap(sim, R, w)
        p, v, ids = sim.download_local()
        check_record(g, a, p, v, ids, n, R, w, dx)
        return dict(g=g, a=a, p=p, v=v, ids=ids, dead=entries(fs, sim) - len(p), removed=sim.source_stats()["removed_last"])

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), "decomposed", work)
    cat = lambda key: np.concatenate([r[key] for r in res])                # noqa: E731
    assert res[0]["removed"] > 0 and len(cat("p")) == len(pos) - res[0]["removed"]
    assert all(r["dead"] > 0 for r in res)
    grid, attr = check_merged(fs, [r["g"] for r in res], [r["a"] for r in res], cat("p"), cat("v"), cat("ids"), n, R, w, dx)
    assert np.isin(attr.id[grid.active], cat("ids")).all()                 # no removed particle owns a voxel


@pytest.mark.parametrize("mode", MODES)
def test_snapshots_survive_moving_cut_planes(fs, mode):
    """The scene of test_gpu_dist_sdf.py's test of this name.  Every step is preceded by an attribute snapshot that is waited for
    only after the step; around the step that moves the planes both records are held against the particles of their own moment."""
    fd = fs.load_dist()
    n, steps, dims, (R, w, dx) = 32, 8, (2, 2, 2), (1.0, 1.0, 1.0)
    pos = fs.water_cube_drop(n, 2, seed=0)
    vel = np.random.default_rng(1).standard_normal(pos.shape) * 0.3
    pos = pos + np.array([3.5, 4.5, -2.5])
    solid = np.zeros((n, n, n), dtype=np.uint8)
    solid[:2] = solid[-2:] = 1; solid[:, :2] = solid[:, -2:] = 1; solid[:, :, :2] = solid[:, :, -2:] = 1

    def work(sim, r):
        sim.set_solid(solid)
        sim.upload_global(pos, vel)
        sim.set_rebalance(4, 1.3)
        moved, checked = [], None
        for k in range(steps):
            before = sim.download_local() if checked is None else None
            sim.sdf_snapshot(R, w, attr=True)                               # outstanding across the step
            st = sim.step()
            moved.append(bool(st["paths"] & REBALANCED))
            gc, pc = fs.SdfGridC(), fs.SdfAttrPartC()
            fs.check(fs.lib.fluid_dist_sdf_wait_attr(sim._h, C.byref(gc), C.byref(pc)))
            if not moved[-1] or checked is not None:
                continue
            g, a = view(fs, gc), view_part(pc)                              # the handle's own pinned memory, not a copy
            if g.n_leaves:
                check_record(g, a, *before, n, R, w, dx)                    # taken from the old window's handle
            else:
                assert len(before[0]) == 0
            keep = None if not g.n_leaves else (g.values.copy(), a.id.copy(), a.velocity.copy(), a.dist2.copy())
            rec = (a.id.copy(), a.velocity.copy(), a.dist2.copy()) if g.n_leaves else (np.empty((0, 512)), np.empty((0, 3, 512)), np.empty((0, 512)))
            ga = (fs.SdfGrid(g.n, g.origin.copy(), g.values.copy(), g.active, g.background, g.radius, g.half_width), fs.SdfAttrPart(*rec))
            now = sim.download_local()
            gb = snap(sim, R, w)                                            # the particles as the new window holds them
            check_record(*gb, *now, n, R, w, dx)
            if keep:                                                        # promised until the second following snapshot
                assert np.array_equal(u32(g.values), u32(keep[0])) and np.array_equal(a.id, keep[1])
                assert np.array_equal(u32(a.velocity), u32(keep[2])) and np.array_equal(u32(a.dist2), u32(keep[3]))
            checked = dict(k=k, a=ga, b=gb, before=before, now=now)
        return moved, checked

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), mode, work, dx=dx)
    moved = res[0][0]
    assert any(moved) and all(r[0] == moved for r in res)
    assert all(r[1] is not None and r[1]["k"] == moved.index(True) for r in res)
    assert any(r[1]["a"][0].n_leaves > 0 for r in res)
    for key, ps in (("a", "before"), ("b", "now")):
        p, v, ids = (np.concatenate([r[1][ps][j] for r in res]) for j in range(3))
        check_merged(fs, [r[1][key][0] for r in res], [r[1][key][1] for r in res], p, v, ids, n, R, w, dx)


def test_slots_refusals_and_stats(fs):
    """Two blocks along x, every particle in the first: the second rank's record is empty."""
    fd = fs.load_dist()
    n, dims, (R, w, dx) = 24, (2, 1, 1), SETS[0]
    pos = block((3, 3, 3), 2, 9, centre=(-7, 0, 0))
    vel = attr_ref.velocities(pos) * 0.1

    def work(sim, r):
        h = sim._h
        prm = fs.SdfParams(R, w)
        g, pc = fs.SdfGridC(), fs.SdfAttrPartC()
        assert fs.lib.fluid_dist_sdf_wait_attr(h, C.byref(g), C.byref(pc)) == ERR_STATE     # nothing outstanding
        assert fs.lib.fluid_dist_sdf_wait_attr(h, None, C.byref(pc)) == ERR_ARG
        for bad in ((2.0, 2.5), (1.5, 0.5), (0.0, 2.0), (float("nan"), 2.0)):
            assert fs.lib.fluid_dist_sdf_snapshot_attr(h, C.byref(fs.SdfParams(*bad))) == ERR_ARG, bad
        assert fs.lib.fluid_dist_sdf_snapshot_attr(h, None) == ERR_ARG
        assert fs.lib.fluid_dist_sdf_snapshot_attr(None, C.byref(prm)) == ERR_ARG
        assert fs.lib.fluid_dist_sdf_wait_attr(None, C.byref(g), C.byref(pc)) == ERR_ARG
        assert fs.lib.fluid_dist_sdf_wait(h, C.byref(g)) == ERR_STATE                       # a refused snapshot is not outstanding
        sim.upload_global(pos, vel)
        me = sim.download_local()
        # a third outstanding snapshot is refused, whatever its kind
        sim.sdf_snapshot(R, w, attr=True)
        sim.sdf_snapshot(R, w)
        assert fs.lib.fluid_dist_sdf_snapshot_attr(h, C.byref(prm)) == ERR_STATE
        assert fs.lib.fluid_dist_sdf_snapshot(h, C.byref(prm)) == ERR_STATE
        assert "two level-set snapshots" in fs.lib.fluid_last_error().decode()
        # fluid_dist_sdf_wait on an attribute snapshot: the geometry alone; _wait_attr on a plain one: NULL record pointers
        ga, gp = fs.SdfGridC(), fs.SdfGridC()
        fs.check(fs.lib.fluid_dist_sdf_wait(h, C.byref(ga)))
        fs.check(fs.lib.fluid_dist_sdf_wait_attr(h, C.byref(gp), C.byref(pc)))
        assert pc.n_leaves == gp.n_leaves and not pc.id and not pc.velocity and not pc.dist2
        va, vp = view(fs, ga), view(fs, gp)
        assert same_geometry(va, vp)
        st = sim.sdf_stats()                                                                # of the last snapshot: the plain one
        assert st["leaves_listed"] == gp.n_leaves and st["bytes_to_host"] == gp.n_leaves * LEAF_BYTES + 4
        assert fs.lib.fluid_dist_sdf_wait_attr(h, C.byref(g), C.byref(pc)) == ERR_STATE
        # attribute, then plain, then attribute again through the same two slots: each has its own bytes and stats
        g1, a1 = snap(sim, R, w)
        assert sim.sdf_stats()["bytes_to_host"] == g1.n_leaves * (LEAF_BYTES + PART_BYTES) + 4
        sim.sdf_snapshot(R, w)
        g2 = sim.sdf_wait()
        assert sim.sdf_stats()["bytes_to_host"] == g2.n_leaves * LEAF_BYTES + 4
        g3, a3 = snap(sim, R, w)
        assert same_geometry(g1, g2) and same_geometry(g1, g3) and same_geometry(g1, vp)
        assert np.array_equal(a1.id, a3.id) and np.array_equal(u32(a1.dist2), u32(a3.dist2))
        if r == 1:                                                         # no particle: no leaf, NULL pointers, the count alone travels
            assert g1.n_leaves == 0 and a1.n_leaves == 0 and len(me[0]) == 0
            sim.sdf_snapshot(R, w, attr=True)
            fs.check(fs.lib.fluid_dist_sdf_wait_attr(h, C.byref(g), C.byref(pc)))
            assert g.n_leaves == 0 and pc.n_leaves == 0 and not pc.id and not pc.velocity and not pc.dist2 and not g.values
            assert sim.sdf_stats()["bytes_to_host"] == 4
        else:
            check_record(g1, a1, *me, n, R, w, dx)
        return len(me[0])

    res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), "decomposed", work)
    assert res == [len(pos), 0]


def test_snapshots_do_not_disturb_the_steps(fs):
    fd = fs.load_dist()
    n, dims, (R, w, _) = 32, (2, 2, 2), SETS[0]
    pos = fs.water_cube_drop(n, 4, seed=3)

    def work(take):
        def body(sim, r):
            sim.upload_global(pos)
            stats = []
            for _ in range(4):
                stats.append(sim.step())
                if take:
                    sim.sdf_snapshot(R, w, attr=True)
                    sim.sdf_wait_attr()
            p, v, ids = sim.download_local()
            o = np.argsort(ids)
            return stats, p[o].tobytes(), v[o].tobytes(), ids[o].tobytes()
        return body

    cuts = fd.uniform_cuts(n, dims)
    a = run_group(fs, dims, n, cuts, "decomposed", work(False))
    b = run_group(fs, dims, n, cuts, "decomposed", work(True))
    for ra, rb in zip(a, b):
        assert ra[0] == rb[0]
        assert ra[1:] == rb[1:] and len(ra[3]) > 0


@pytest.mark.parametrize("smooth", [None, (1, 2, -0.25)], ids=["raw", "smoothed"])
def test_program_on_blocks_writes_the_mesh(fs, tmp_path, smooth):
    fd = fs.load_dist()
    n, ppc, steps, (R, w, dx), blocks, scale = 32, 2, 3, SETS[0], "2x1x1", 1.0
    outs = {}
    for mode in ("plain", "mesh"):
        extra = dict(FLUID_BLOCKS=blocks, FLUID_BLOCKS_MESH="", FLUID_BLOCKS_MESH_VEL="", FLUID_OUT_SMOOTH="", FLUID_OUT_MESH="", FLUID_OUT_MESH_VEL="")
        if mode == "mesh":                                                 # (an empty value is an unset variable to the program)
            extra.update(FLUID_BLOCKS_MESH=f"{R},{w}", FLUID_BLOCKS_MESH_VEL="1")
            if smooth:
                extra["FLUID_OUT_SMOOTH"] = ",".join(str(x) for x in smooth)
        r = run_fluid(tmp_path / mode, **extra)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["plain"] == outs["mesh"]
    for nm in ["mygrids.vdb"] + [f"simulation/mygrids{i}.vdb" for i in range(steps)]:
        assert leaf_ref.same_file(tmp_path / "plain" / nm, tmp_path / "mesh" / nm), nm
    assert not list((tmp_path / "plain").rglob("*.ply")) and not list((tmp_path / "mesh").rglob("surface*"))
    # the same run here: the program's cut planes, ids and upload
    dims = tuple(int(x) for x in blocks.split("x"))
    pos = fs.water_cube_drop(n, ppc, seed=0)

    def work(sim, r):
        sim.upload_global(pos)
        out = []
        for _ in range(steps):
            sim.step()
            out.append(sim.download_local())
        return out

    res = run_group(fs, dims, n, fd.partition_blocks(n, pos, dims), None, work)
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        p, v, ids = (np.concatenate([r[i][j] for r in res]) for j in range(3))
        o = np.argsort(ids)
        p, v, ids = p[o], v[o], ids[o]
        val, act = sdf_ref.closed(p, n, R, w, dx)
        rows, v32 = attr_ref.closest(p, v, n, R, w, dx)                    # sorted by id: the smallest row is the smallest id
        if smooth:
            val = sdf_filter_ref.smooth(val, act, bg, *smooth)
        mv, mq = mesh_ref.mesh(val)[:2]
        vv, _ = attr_ref.vertex_velocity(val, act, v32)
        fv, ff = read_ply(tmp_path / "mesh" / f"simulation/mesh{i}.ply")
        assert fv.shape == (len(mv), 6) and len(mq) > 0
        assert np.array_equal(u32(fv[:, :3]), u32(np.asarray(mv, np.float32) * np.float32(dx))), i
        assert np.array_equal(ff["i"], mq) and (ff["k"] == 4).all(), i
        assert np.array_equal(u32(fv[:, 3:]), u32(vv * np.float32(scale))) and np.abs(vv).max() > 0, i
