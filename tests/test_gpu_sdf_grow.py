"""GPU (-m gpu): the grown band of the liquid surface (fluid_sdf_set_track_grow, kernels_sdf_grow.hip).  In every comparison the
device list equals tests/sdf_grow_ref.py — a reference that knows no leaves and no range — in origins, masks, values as bit
patterns, ids and velocity bits, and equals the host function's (fluid_sdf_filter_grown) of the unfiltered list; the device mesh
equals tests/mesh_ref.py of the grown field and fluid_sdf_mesh* of the grown list; the image equals fluid_sdf_render of it."""
import ctypes as C

import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_grow_ref as G
import sdf_ref
import sdf_track_ref
from sdf_testlib import read_ply, run_fluid, same_attr, same_grid, same_mesh, u32

pytestmark = pytest.mark.gpu

SETS = [(2.0, 2.0, 1.0), (1.5, 2.5, 1.0), (1.0, 2.0, 0.5)]
SCENES = ["one", "corner", "lo", "hi", "cloud", "faces"]
ERR_ARG, ERR_STATE = 1, 3
NO_ID = 0xFFFFFFFF


def filt_of(case, dx):
    return (case[0], case[1], case[2] * dx), case[3]


def leaves_of(dense, bg):
    """(origin, values, active, ids, velocities) of a dense (val, act, ids, vel32)."""
    vt, at, it, velt = dense
    org, v, a = sdf_ref.leaf_list(vt, at, bg)
    li, lv = attr_ref.leaf_attr(it, velt, org)
    return org, v, a, li, lv


def check(fs, sim, dense, bg, plain, plain_attr, R, w, dx, case, what=""):
    """With growing on and the case's tracking set: the handle's filtered surface (with and without attributes), its mesh and its
    attribute mesh are the reference's `dense` = (val, act, ids, vel32) and the host functions' of the unfiltered list `plain`."""
    what = f"{what} {(R, w, dx)} {case}"
    org, v, a, li, lv = leaves_of(dense, bg)
    filt, N = filt_of(case, dx)
    sim.sdf_set_track(N, True, grow=True)
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g, at = sim.sdf_wait_attr()
    assert g.n_leaves == len(org) and np.array_equal(g.origin, org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what
    same_attr(at, li, lv, what)
    sim.sdf_snapshot(R, w, smooth=filt)
    g2 = sim.sdf_wait()
    same_grid(g2, g, what + " (without attributes)")
    assert sim.sdf_stats()["leaves_listed"] == len(org)
    host, hat = fs.sdf_filter_grown(plain, filt, N, attr=plain_attr)
    same_grid(g, host, what + " (host function)")
    same_attr(at, hat.id, hat.velocity, what + " (host function)")
    ref = mesh_ref.mesh(dense[0])
    sim.mesh_snapshot(R, w, smooth=filt)
    got = sim.mesh_wait()
    same_mesh(got, ref[0], ref[1], what)
    hm = fs.sdf_mesh(host)
    same_mesh(got, hm.vertices, hm.quads, what + " (host mesher)")
    sim.mesh_snapshot(R, w, smooth=filt, attr=True)
    mv, mq, mvel = sim.mesh_wait_attr()
    same_mesh((mv, mq), ref[0], ref[1], what + " (attribute mesh)")
    if len(ref[0]):
        vv, _ = attr_ref.vertex_velocity(dense[0], dense[1], dense[3])
        assert np.array_equal(u32(mvel), u32(vv)), what
        assert np.array_equal(u32(mvel), u32(fs.sdf_mesh_attr(host, hat))), what + " (host vertex velocities)"
    else:
        assert mvel is None, what
    return g, got


def start(fs, name, n, R, w, dx):
    """(handle with the scene's particles, bg, the unfiltered list and its attributes)."""
    pos, vel, _, _, _, _, bg = G.base(name, n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    sim.sdf_snapshot(R, w, attr=True)
    plain, plain_attr = sim.sdf_wait_attr()
    assert plain.n_leaves > 0
    return sim, bg, plain, plain_attr


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [20, 32])
@pytest.mark.parametrize("name", SCENES)
def test_grown_surface_attributes_and_mesh_are_the_reference(fs, name, n, R, w, dx):
    """Every case of GROWS on ONE handle, one after the other: lists that grow, shrink and become empty (the snapshot after an empty
    one works).  n = 20: the grid [-10, 9] is no multiple of 8 and its leaves begin at -16."""
    sim, bg, plain, plain_attr = start(fs, name, n, R, w, dx)
    cases = list(G.GROWS)
    if name == "faces":
        cases.append((1, 0, -4.0, 3))                                            # at n = 20 into the grid's hi face: an open mesh
    emptied = 0
    for case in cases:
        g, got = check(fs, sim, G.scene(name, n, R, w, dx, case), bg, plain, plain_attr, R, w, dx, case, f"{name} {n}")
        emptied += g.n_leaves == 0
        if (name, n, R, case) == ("faces", 20, 2.0, (1, 0, -3.0, 3)):
            assert (plain.n_leaves, g.n_leaves) == (1, 19)                       # flagged leaves that the search never listed
        if (name, n, R, case) == ("faces", 20, 2.0, (1, 0, -4.0, 3)):
            assert len(got[1]) > 0 and not mesh_ref.is_closed(got[1])
    assert emptied >= 1 or name == "cloud"
    sim.sdf_snapshot(R, w, attr=True)                                            # unfiltered snapshots are untouched by the setting
    g, at = sim.sdf_wait_attr()
    same_grid(g, plain, "unfiltered with growing set")
    same_attr(at, plain_attr.id, plain_attr.velocity)
    sim.close()


@pytest.mark.parametrize("R,w", [(3.0, 1.0), (2.0, 1.0)])
def test_block_band_walks_inwards_through_the_interior(fs, R, w):
    """The 13^3 block: offsets of +1, +2 and +3 dx activate inactive -bg voxels and unlist whole leaves; +2 and +3 are beyond bg."""
    n, dx = 32, 1.0
    sim, bg, plain, plain_attr = start(fs, "block", n, R, w, dx)
    for case in G.BLOCK_GROWS + [(1, 1, -3.0, 3), (2, 2, -4.0, 2)]:
        g, got = check(fs, sim, G.scene("block", n, R, w, dx, case), bg, plain, plain_attr, R, w, dx, case, "block")
        if case[2] > 0:
            assert 0 < g.n_leaves < plain.n_leaves and mesh_ref.is_closed(got[1])
            assert abs(float(np.abs(got[0]).max()) - (R + 6 - case[2])) <= 0.5
    sim.close()


@pytest.mark.parametrize("name,n,case", [("cloud", 20, (1, 0, -3.0, 3)), ("faces", 20, (1, 0, -4.0, 3)), ("block", 32, (1, 0, 2.0, 3))])
def test_render_normals_and_triangles_of_the_grown_level_set(fs, name, n, case):
    """fluid_render_snapshot and fluid_mesh_snapshot_ex go through the same front half with the range of 5 + T cells: the image is
    fluid_sdf_render of the grown list in hits, depth, normals and rgb; normals and triangles are the host functions' of it."""
    R, w, dx = (3.0, 1.0, 1.0) if name == "block" else SETS[0]
    sim, bg, plain, plain_attr = start(fs, name, n, R, w, dx)
    filt, N = filt_of(case, dx)
    sim.sdf_set_track(N, True, grow=True)
    sim.sdf_snapshot(R, w, smooth=filt)
    g = sim.sdf_wait()
    org, v, a, _, _ = leaves_of(G.scene(name, n, R, w, dx, case), bg)
    assert np.array_equal(g.origin, org) and np.array_equal(u32(g.values), u32(v)) and np.array_equal(g.active, a)
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=48, height=32)
    sim.render_snapshot(R, w, cam, smooth=filt, depth=True, normals=True)
    img = sim.render_wait()
    host = fs.sdf_render(g, cam, None, True, True, True)
    assert img["n_hit"] == host["n_hit"] > 50
    assert np.array_equal(img["rgb"], host["rgb"]) and np.array_equal(u32(img["depth"]), u32(host["depth"]))
    assert np.array_equal(u32(img["normals"]), u32(host["normals"]))
    sim.sdf_set_track(N, True, grow=False)
    if abs(case[2] * dx) <= float(bg):
        sim.render_snapshot(R, w, cam, smooth=filt, depth=True)
        assert not np.array_equal(u32(sim.render_wait()["depth"]), u32(img["depth"]))   # the dilation did something to the image
    sim.sdf_set_track(N, True, grow=True)
    ref = mesh_ref.mesh(G.scene(name, n, R, w, dx, case)[0])
    sim.mesh_snapshot(R, w, smooth=filt, attr=True, normals=True, triangles=True)
    mv, mq, parts = sim.mesh_wait_ex()
    same_mesh((mv, mq), ref[0], ref[1])
    assert len(mv) > 0 and np.array_equal(u32(parts["normals"]), u32(fs.sdf_mesh_normals(g)))
    assert np.array_equal(parts["triangles"], fs.mesh_triangles(mv, mq))
    host_g, host_a = fs.sdf_filter_grown(plain, filt, N, attr=plain_attr)
    assert np.array_equal(u32(parts["velocity"]), u32(fs.sdf_mesh_attr(host_g, host_a)))
    sim.close()


def test_stale_scratch_and_growing_on_and_off(fs):
    """The cloud, grown by 3 voxels, comes first: at n = 20 it fills the grid's 64 leaves and writes both value buffers, both sets
    of masks and flags, the list flags and the attributes.  Then single particles far from it on the same handle, growing on and
    off in alternation: nothing may read what the first run left.  Growing off in between gives today's tracked bytes."""
    n, (R, w, dx) = 20, SETS[0]
    first = (1, 0, -3.0, 3)
    sim, bg, plain, plain_attr = start(fs, "cloud", n, R, w, dx)
    cloud = G.scene("cloud", n, R, w, dx, first)
    g, _ = check(fs, sim, cloud, bg, plain, plain_attr, R, w, dx, first, "cloud")
    assert g.n_leaves == 64 > plain.n_leaves
    rng = np.random.default_rng(3)
    for p in ([[9.3, 9.2, -9.6]], [[0.3, -0.2, 0.41]], [[9.3, 9.2, -9.6], [-9.9, -9.7, 9.1]], [[-9.6, 3.5, 3.5]]):
        pos = np.array(p)
        vel = rng.uniform(-3, 3, pos.shape)
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        ids, v32 = attr_ref.closest(pos, vel, n, R, w, dx)
        for case in ((1, 0, -3.0, 3), (1, 1, 0.0, 3), (1, 0, 1.0, 2)):
            sim.upload_particles(pos, vel)
            sim.sdf_snapshot(R, w, attr=True)
            pl, pla = sim.sdf_wait_attr()
            assert pl.n_leaves <= 16
            W, K, units, N = case
            dense = G.grown(val, act, bg, dx, W, K, units * dx, N, ids, v32)
            check(fs, sim, dense, bg, pl, pla, R, w, dx, case, f"particles {p} after the cloud")
            sim.sdf_set_track(N, True, grow=False)                               # on -> off: the tracked bytes, and its offset limit
            if abs(units * dx) <= float(bg):
                vt, at = sdf_track_ref.tracked(val, act, bg, dx, W, K, units * dx, N, True)
                org, v, a = sdf_ref.leaf_list(vt, at, bg)
                sim.sdf_snapshot(R, w, smooth=(W, K, units * dx))
                t = sim.sdf_wait()
                assert np.array_equal(t.origin, org) and np.array_equal(u32(t.values), u32(v)) and np.array_equal(t.active, a), (p, case)
                host, _ = fs.sdf_filter_tracked(pl, (W, K, units * dx), N)
                same_grid(t, host, "growing off: the tracked host function")
                sim.mesh_snapshot(R, w, smooth=(W, K, units * dx))
                mt = mesh_ref.mesh(vt)
                same_mesh(sim.mesh_wait(), mt[0], mt[1], "growing off")
            else:
                with pytest.raises(fs.FluidError):
                    sim.sdf_snapshot(R, w, smooth=(W, K, units * dx))
        sim.upload_particles(*G.base("cloud", n, R, w, dx)[:2])
        check(fs, sim, cloud, bg, plain, plain_attr, R, w, dx, first, "cloud again")
    sim.close()


def test_settings_slots_and_refusals(fs):
    n, (R, w, dx) = 32, SETS[0]
    sim = fs.FluidSim(n=n)
    h = sim._h
    prm = fs.SdfParams(R, w)
    ok = fs.SdfFilter(1, 1, 0.0)
    g = fs.SdfGridC()
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim.upload_particles(pos)
    for bad in (2, -1, 256):
        assert fs.lib.fluid_sdf_set_track_grow(h, bad) == ERR_ARG, bad
    assert fs.lib.fluid_sdf_set_track_grow(None, 1) == ERR_ARG
    with pytest.raises(fs.FluidError):
        sim.sdf_set_track(3, True, grow=2)
    sim.sdf_set_track(None)
    sim.sdf_snapshot(R, w, smooth=(1, 1, 3.0))                                   # the refused values left growing off
    assert sim.sdf_wait().n_leaves > 0
    # growing with tracking off, with N = 0 or without the trim: FLUID_ERR_ARG from every filtered snapshot, in either order of the setters
    assert fs.lib.fluid_sdf_set_track_grow(h, 1) == 0
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=16, height=8)
    for setting in (None, (0, True), (3, False), (0, False)):
        if setting is None:
            assert fs.lib.fluid_sdf_set_track(h, None) == 0
        else:
            assert fs.lib.fluid_sdf_set_track(h, C.byref(fs.SdfTrack(setting[0], int(setting[1]), 0))) == 0
        assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_ARG, setting
        assert "normalize >= 1 and trim = 1" in fs.lib.fluid_last_error().decode()
        assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_ARG
        assert fs.lib.fluid_sdf_snapshot_attr(h, C.byref(prm), C.byref(ok)) == ERR_ARG
        assert fs.lib.fluid_mesh_snapshot_ex(h, C.byref(prm), C.byref(ok), 2) == ERR_ARG
        assert fs.lib.fluid_render_snapshot(h, C.byref(prm), C.byref(ok), C.byref(cam), None, 1) == ERR_ARG
        assert fs.lib.fluid_sdf_snapshot(h, C.byref(prm)) == 0                   # an unfiltered snapshot is untouched
        assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == 0 and g.n_leaves > 0
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE                     # none of the refused calls left a snapshot behind
    assert fs.lib.fluid_sdf_set_track_grow(h, 0) == 0                            # growing off: the settings above are fine again
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == 0 and fs.lib.fluid_sdf_wait(h, C.byref(g)) == 0
    # the offset limit: 4 dx, not bg
    sim.sdf_set_track(3, True, grow=True)
    four = float(np.float32(4.0) * np.float32(dx))
    above = float(np.nextafter(np.float32(four), np.float32(np.inf)))
    for sign in (1.0, -1.0):
        f = fs.SdfFilter(1, 0, sign * above)
        assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(f)) == ERR_ARG
        assert "4 dx" in fs.lib.fluid_last_error().decode()
        assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(f)) == ERR_ARG
        f = fs.SdfFilter(1, 0, sign * four)
        assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(f)) == 0
        assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == 0
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE
    # two outstanding snapshots, a step in between, the third refused as before
    c1, c2 = (1, 1, -3.0, 3), (2, 1, 1.0, 2)
    sim.sdf_snapshot(R, w, smooth=filt_of(c1, dx)[0])
    sim.mesh_snapshot(R, w, smooth=filt_of(c1, dx)[0])
    sim.step()
    p2, _ = sim.download_particles()
    sim.sdf_set_track(c2[3], True, grow=True)
    sim.sdf_snapshot(R, w, smooth=filt_of(c2, dx)[0])
    sim.mesh_snapshot(R, w, smooth=filt_of(c2, dx)[0])
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE
    assert "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE
    ga, gb = sim.sdf_wait(), sim.sdf_wait()
    ma, mb = sim.mesh_wait(), sim.mesh_wait()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE
    bg = sdf_ref.constants(R, w, dx)[3]
    for got, m, p, case in ((ga, ma, pos, c1), (gb, mb, p2, c2)):
        val, act = sdf_ref.closed(p, n, R, w, dx)
        vt, at = G.grown(val, act, bg, dx, case[0], case[1], case[2] * dx, case[3])
        org, v, a = sdf_ref.leaf_list(vt, at, bg)
        assert np.array_equal(got.origin, org) and np.array_equal(u32(got.values), u32(v)) and np.array_equal(got.active, a), case
        ref = mesh_ref.mesh(vt)
        same_mesh(m, ref[0], ref[1], str(case))
        assert len(ref[0]) > 0
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    for v in (1, 0):
        assert fs.lib.fluid_sdf_set_track_grow(sim._h, v) == ERR_STATE
        assert "fluid_sdf_filter_grown" in fs.lib.fluid_last_error().decode()
    with pytest.raises(fs.FluidError) as e:
        sim.sdf_set_track(3, True, grow=True)
    assert e.value.code == ERR_STATE and "fluid_sdf_filter_grown" in str(e.value)
    sim.close()
    grp.close()


def test_all_four_snapshots_in_one_step_with_growing_on(fs):
    """The same input on two handles: B takes density, grown surface, grown mesh and grown image snapshots after every step, A the
    density alone.  Particles bit for bit, the step stats and the density lists as on A; B's surface is the reference's of its
    particles, its mesh the mesh reference's, its image fluid_sdf_render of its list."""
    n, (R, w, dx) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=3)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    for s in (a, b):
        s.upload_particles(pos)
    b.sdf_set_track(3, True, grow=True)
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=48, height=32)
    bg = sdf_ref.constants(R, w, dx)[3]
    sa, sb = [], []
    for k in range(3):
        sa.append(a.step())
        sb.append(b.step())
        case = [(1, 1, -3.0, 3), (1, 0, 1.0, 3), (2, 1, -0.25, 3)][k]
        filt = filt_of(case, dx)[0]
        a.output_snapshot()
        b.output_snapshot()
        b.sdf_snapshot(R, w, smooth=filt)
        b.mesh_snapshot(R, w, smooth=filt)
        b.render_snapshot(R, w, cam, smooth=filt, depth=True, normals=True)
        da, db = a.output_wait(), b.output_wait()
        assert np.array_equal(da.origin, db.origin) and np.array_equal(u32(da.values), u32(db.values)) and da.n_leaves > 0
        g = b.sdf_wait()
        v, q = b.mesh_wait()
        img = b.render_wait()
        p, _ = b.download_particles()
        val, act = sdf_ref.closed(p, n, R, w, dx)
        vt, at = G.grown(val, act, bg, dx, case[0], case[1], case[2] * dx, case[3])
        org, lv, la = sdf_ref.leaf_list(vt, at, bg)
        assert g.n_leaves > 0 and np.array_equal(g.origin, org) and np.array_equal(u32(g.values), u32(lv)) and np.array_equal(g.active, la), case
        ref = mesh_ref.mesh(vt)
        same_mesh((v, q), ref[0], ref[1], str(case))
        host = fs.sdf_render(g, cam, None, True, True, True)
        assert img["n_hit"] == host["n_hit"] > 20 and np.array_equal(img["rgb"], host["rgb"])
        assert np.array_equal(u32(img["depth"]), u32(host["depth"])) and np.array_equal(u32(img["normals"]), u32(host["normals"]))
    assert sa == sb
    (pa, va), (pb, vb) = a.download_particles(), b.download_particles()
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    for s in (a, b):
        s.close()


def test_blocks_grow_the_merged_list(fs):
    """A decomposed run after 2 steps: the host grown filter of the merged rank lists is the one-GPU handle's grown snapshot of the
    same particles, and the host mesher of it is that handle's grown mesh."""
    fd = fs.load_dist()
    n, (R, w, dx), dims = 32, SETS[0], (2, 1, 1)
    pos = fs.water_cube_drop(n, 4, seed=1)
    grp = fd.LocalGroup(2)
    sims = [None] * 2

    def run(r):
        sim = fd.DistFluidSim(n, dims, fd.uniform_cuts(n, dims), grp.comms[r])
        sims[r] = sim
        sim.upload_global(pos)
        for _ in range(2):
            sim.step()
        sim.sdf_snapshot(R, w)
        return sim.sdf_wait(), sim.download_local()[0]

    try:
        res = grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    merged = fs.merge_sdf_grids([r[0] for r in res])
    allp = np.concatenate([r[1] for r in res])
    one = fs.FluidSim(n=n)
    one.upload_particles(allp)
    for case in ((1, 2, -3.0, 3), (2, 1, 1.0, 2)):
        filt, N = filt_of(case, dx)
        host = fs.sdf_filter_grown(merged, filt, N)
        one.sdf_set_track(N, True, grow=True)
        one.sdf_snapshot(R, w, smooth=filt)
        g = one.sdf_wait()
        assert g.n_leaves > 8
        same_grid(host, g, f"blocks {case}")
        hm = fs.sdf_mesh(host)
        one.mesh_snapshot(R, w, smooth=filt)
        v, q = one.mesh_wait()
        assert len(q) > 100
        same_mesh((hm.vertices, hm.quads), v, q, f"blocks {case}")
    one.close()


def test_driver_writes_the_grown_mesh_on_one_gpu_and_on_blocks(fs, tmp_path):
    """The `fluid` program with FLUID_OUT_SMOOTH=1,1,-3 — an offset beyond bg = 2, which FLUID_OUT_TRACK=3 alone refuses — and
    FLUID_OUT_TRACK=3,1,1: on one GPU mesh<i>.ply is the handle's grown mesh of step i; FLUID_BLOCKS=2x1x1 writes the same mesh
    through fluid_sdf_filter_grown of the merged lists, and with FLUID_BLOCKS_MESH_VEL a velocity per vertex beside it."""
    n, ppc, steps, (R, w, dx) = 24, 4, 2, SETS[0]
    common = dict(FLUID_OUT_SMOOTH="1,1,-3", FLUID_OUT_TRACK="3,1,1")
    plain = run_fluid(tmp_path / "plain", n, ppc, steps, FLUID_OUT_MESH=f"{R},{w}", FLUID_OUT_SMOOTH="1,1,-1")
    one = run_fluid(tmp_path / "one", n, ppc, steps, FLUID_OUT_MESH=f"{R},{w}", **common)
    assert plain == one                                                          # stdout is what it is without the variable
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    sim.sdf_set_track(3, True, grow=True)
    bg = sdf_ref.constants(R, w, dx)[3]
    meshes = []
    for i in range(steps):
        sim.step()
        sim.mesh_snapshot(R, w, smooth=(1, 1, -3.0))
        v, q = sim.mesh_wait()
        fv, fq, _ = read_ply(tmp_path / "one" / f"simulation/mesh{i}.ply")
        assert len(q) > 0 and np.array_equal(u32(fv), u32(v * np.float32(dx))) and np.array_equal(fq, q), i
        meshes.append((v, q))
    p, _ = sim.download_particles()
    val, act = sdf_ref.closed(p, n, R, w, dx)
    ref = mesh_ref.mesh(G.grown(val, act, bg, dx, 1, 1, -3.0 * dx, 3)[0])        # ... and the last one is the reference's
    same_mesh(meshes[-1], ref[0], ref[1])
    sim.close()
    run_fluid(tmp_path / "blocks", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_MESH=f"{R},{w}", **common)
    run_fluid(tmp_path / "vel", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_MESH=f"{R},{w}", FLUID_BLOCKS_MESH_VEL="1", **common)
    for i in range(steps):
        bv, bq, _ = read_ply(tmp_path / "blocks" / f"simulation/mesh{i}.ply")
        vv, vq, extra = read_ply(tmp_path / "vel" / f"simulation/mesh{i}.ply")
        assert np.array_equal(u32(bv), u32(vv)) and np.array_equal(bq, vq) and extra.shape == (len(vv), 3) and np.isfinite(extra).all(), i
        assert extra.any() and len(bq) > 0
        far = np.abs(bv).max() - np.abs(meshes[i][0]).max() * dx                 # (the block solver differs from one GPU in the last bits)
        assert abs(float(far)) < 1.0, i
