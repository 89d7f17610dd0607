"""GPU (-m gpu): the renormalised liquid surface (fluid_sdf_set_track, kernels_sdf_track.hip).  In every comparison the device list
equals tests/sdf_track_ref.py of tests/sdf_ref.py closed() — origins, masks, values as bit patterns — and the host function's
(fluid_sdf_filter_tracked); the device mesh equals tests/mesh_ref.py of the tracked field and fluid_sdf_mesh of the tracked list:
vertices as bit patterns, quads exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_ref
import sdf_filter_ref
import sdf_ref
import sdf_track_ref
from sdf_testlib import fluid_env, read_ply, run_fluid, same_grid, same_mesh, u32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = mesh_ref.SETS
TRACKS = sdf_track_ref.TRACKS
SCENES = ["one", "corner", "lo", "hi", "cloud"]
ERR_ARG, ERR_STATE = 1, 3
LEAF_BYTES = 2048 + 64 + 12
NO_ID = 0xFFFFFFFF


def args_of(case, dx):
    W, K, units, N, tr = case
    return (W, K, units * dx), (N, bool(tr))


def ref_of(pos, n, R, w, dx, case):
    """(leaf list (origin, values, active) of the tracked field, its mesh, the tracked (val, act)) from the numpy references."""
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    bg = sdf_ref.constants(R, w, dx)[3]
    vt, at = sdf_track_ref.tracked(val, act, bg, dx, case[0], case[1], case[2] * dx, case[3], bool(case[4]))
    return sdf_ref.leaf_list(vt, at, bg), mesh_ref.mesh(vt), (vt, at)


def check(fs, sim, leaves, mesh, R, w, dx, case, what=""):
    """With the case's tracking set, the handle's filtered surface list is `leaves` and its filtered mesh is `mesh`."""
    what = f"{what} {case}"
    org, v, a = leaves
    filt, track = args_of(case, dx)
    sim.sdf_set_track(*track)
    sim.sdf_snapshot(R, w, smooth=filt)
    g = sim.sdf_wait()
    assert g.n_leaves == len(org) and np.array_equal(g.origin, org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what
    assert sim.sdf_stats()["leaves_listed"] == len(org) and sim.sdf_stats()["bytes_to_host"] == len(org) * LEAF_BYTES + 4
    sim.mesh_snapshot(R, w, smooth=filt)
    got = sim.mesh_wait()
    same_mesh(got, mesh[0], mesh[1], what)
    return g, got


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", SCENES)
def test_tracked_surface_and_mesh_are_the_reference(fs, name, n, R, w, dx):
    """Every case of TRACKS on one handle, one after the other: lists that keep every leaf, lose some, become empty (and the
    snapshot after an empty one works), the stepped offset, and the tracking that does nothing."""
    sim = fs.FluidSim(n=n, dx=dx)
    pos = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))[0]
    sim.upload_particles(pos)
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    assert plain.n_leaves > 0
    for case in TRACKS:
        _, vt, at, bg, mesh = sdf_track_ref.scene(name, n, R, w, dx, case)
        g, got = check(fs, sim, sdf_ref.leaf_list(vt, at, bg), mesh, R, w, dx, case, name)
        filt, track = args_of(case, dx)
        host, kept = fs.sdf_filter_tracked(plain, filt, track)
        same_grid(g, host, f"host function {case}")
        hm = fs.sdf_mesh(host)
        same_mesh(got, hm.vertices, hm.quads, f"host mesher {case}")
        if case[3] == 0 and case[4] == 0:                                        # the untracked filtered snapshot's bytes
            sim.sdf_set_track(None)
            sim.sdf_snapshot(R, w, smooth=filt)
            same_grid(g, sim.sdf_wait(), "tracking that does nothing")
            sim.mesh_snapshot(R, w, smooth=filt)
            v, q = sim.mesh_wait()
            same_mesh(got, v, q, "tracking that does nothing")
        if (name, n, R, w, case) == ("one", 16, 1.5, 2.5, (4, 3, 0.0, 2, 1)):
            assert g.n_leaves == 0 and len(got[0]) == 0                          # trimmed away: an EMPTY list
        if (name, n, R, w, case) == ("hi", 25, 1.5, 2.5, (1, 1, 0.0, 3, 1)):
            assert (plain.n_leaves, g.n_leaves) == (5, 4) and list(kept) != list(range(5))
    sim.sdf_set_track(3, True)                                                   # unfiltered snapshots are untouched by the setting
    sim.sdf_snapshot(R, w)
    same_grid(sim.sdf_wait(), plain, "unfiltered with tracking set")
    sim.close()


@pytest.mark.parametrize("case", [(1, 1, 0.0, 3, 1), (1, 0, 0.6, 2, 1)])
def test_render_and_normals_of_the_tracked_level_set(fs, case):
    """fluid_render_snapshot and fluid_mesh_snapshot_ex with normals go through the same front half: the image is fluid_sdf_render
    of the tracked list, the normals are fluid_sdf_mesh_normals of it."""
    n, (R, w, dx) = 25, SETS[3]
    pos = mesh_ref.positions("cloud", n)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    filt, track = args_of(case, dx)
    sim.sdf_set_track(*track)
    sim.sdf_snapshot(R, w, smooth=filt)
    g = sim.sdf_wait()
    leaves, mesh, _ = ref_of(pos, n, R, w, dx, case)
    assert np.array_equal(g.origin, leaves[0]) and np.array_equal(u32(g.values), u32(leaves[1])) and g.n_leaves < 61
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=48, height=32)
    sim.render_snapshot(R, w, cam, smooth=filt, depth=True, normals=True)
    img = sim.render_wait()
    host = fs.sdf_render(g, cam, None, True, True, True)
    assert img["n_hit"] == host["n_hit"] > 50
    assert np.array_equal(img["rgb"], host["rgb"]) and np.array_equal(u32(img["depth"]), u32(host["depth"]))
    assert np.array_equal(u32(img["normals"]), u32(host["normals"]))
    sim.sdf_set_track(None)
    sim.render_snapshot(R, w, cam, smooth=filt, depth=True)
    assert not np.array_equal(u32(sim.render_wait()["depth"]), u32(img["depth"]))   # the tracking did something to the image
    sim.sdf_set_track(*track)
    sim.mesh_snapshot(R, w, smooth=filt, normals=True, triangles=True)
    v, q, parts = sim.mesh_wait_ex()
    same_mesh((v, q), mesh[0], mesh[1])
    assert len(v) > 500 and np.array_equal(u32(parts["normals"]), u32(fs.sdf_mesh_normals(g)))
    assert np.array_equal(parts["triangles"], fs.mesh_triangles(v, q))
    sim.close()


def test_attributes_of_a_trimmed_snapshot(fs):
    """NO_ID and +0 exactly on the voxels the reference deactivates; ids and velocities elsewhere are the untracked attribute
    snapshot's; the attribute mesh is the host's of the tracked list with the gathered attributes."""
    n, (R, w, dx), case = 25, SETS[0], (1, 1, 0.0, 3, 1)
    pos = mesh_ref.positions("cloud", n)
    vel = np.random.default_rng(11).uniform(-3, 3, pos.shape)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    filt, track = args_of(case, dx)
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g0, a0 = sim.sdf_wait_attr()
    sim.sdf_set_track(*track)
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g1, a1 = sim.sdf_wait_attr()
    leaves, _, _ = ref_of(pos, n, R, w, dx, case)
    assert np.array_equal(g1.origin, leaves[0]) and np.array_equal(u32(g1.values), u32(leaves[1])) and np.array_equal(g1.active, leaves[2])
    assert (g0.n_leaves, g1.n_leaves) == (61, 60)
    sim.sdf_set_track(None)
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    sim.sdf_set_track(*track)
    assert np.array_equal(plain.origin, g0.origin) and np.array_equal(plain.active, g0.active)   # the untracked filter keeps the topology
    host, kept = fs.sdf_filter_tracked(plain, filt, track)
    same_grid(g1, host)
    gone = g0.active[kept] & ~g1.active
    assert gone.sum() > 100 and not (g1.active & ~g0.active[kept]).any()
    assert (a1.id[gone] == NO_ID).all() and (a1.id[~g1.active] == NO_ID).all() and (a1.id[g1.active] != NO_ID).all()
    assert np.array_equal(a1.id[g1.active], a0.id[kept][g1.active])
    v1, v0 = a1.velocity.transpose(0, 2, 1), a0.velocity[kept].transpose(0, 2, 1)
    assert (u32(v1[~g1.active]) == 0).all()                                      # +0, not -0
    assert np.array_equal(u32(v1[g1.active]), u32(v0[g1.active]))
    sim.mesh_snapshot(R, w, smooth=filt, attr=True)
    v, q, mv = sim.mesh_wait_attr()
    hm = fs.sdf_mesh(g1)
    same_mesh((v, q), hm.vertices, hm.quads)
    assert len(v) > 0 and np.array_equal(u32(mv), u32(fs.sdf_mesh_attr(g1, a1)))
    sim.close()


def test_stale_scratch_and_tracking_on_and_off(fs):
    """The cloud, tracked, writes both value buffers, the masks and the list flags; then single particles far from where the
    cloud's leaves were, on the same handle: the leaves of the new range that no particle reaches keep the cloud's values, masks
    and list flags — nothing may read them.  Tracking off in between gives the untracked bytes again."""
    n, (R, w, dx) = 25, (1.0, 1.0, 1.0)
    pos = mesh_ref.positions("cloud", n)
    case = (1, 1, 0.0, 3, 1)
    cl, cm, _ = ref_of(pos, n, R, w, dx, case)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    check(fs, sim, cl, cm, R, w, dx, case, "cloud")
    for p in ([[10.3, 10.2, -9.6]], [[0.3, -0.2, 0.41]], [[10.3, 10.2, -9.6], [-10.4, -9.7, 10.1]]):
        one = np.array(p)
        for c2 in ((1, 1, 0.0, 3, 1), (1, 2, 0.0, 2, 1), (1, 0, 0.6, 2, 1)):
            sim.upload_particles(one)
            l1, m1, _ = ref_of(one, n, R, w, dx, c2)
            assert len(l1[0]) < 30
            check(fs, sim, l1, m1, R, w, dx, c2, f"particles {p} after the cloud")
            sim.sdf_set_track(None)                                              # on -> off: the untracked bytes
            val, act = sdf_ref.closed(one, n, R, w, dx)
            bg = sdf_ref.constants(R, w, dx)[3]
            filt = args_of(c2, dx)[0]
            vf = sdf_filter_ref.smooth(val, act, bg, *filt)
            org, v, a = sdf_ref.leaf_list(vf, act, bg)
            sim.sdf_snapshot(R, w, smooth=filt)
            g = sim.sdf_wait()
            assert np.array_equal(g.origin, org) and np.array_equal(u32(g.values), u32(v)) and np.array_equal(g.active, a)
            sim.mesh_snapshot(R, w, smooth=filt)
            mf = mesh_ref.mesh(vf)
            same_mesh(sim.mesh_wait(), mf[0], mf[1], "off again")
            sim.upload_particles(pos)
            check(fs, sim, cl, cm, R, w, dx, case, "cloud again")
    sim.close()


def test_slots_and_refusals(fs):
    n, (R, w, dx) = 32, SETS[0]
    sim = fs.FluidSim(n=n)
    h = sim._h
    prm = fs.SdfParams(R, w)
    ok = fs.SdfFilter(1, 1, 0.0)
    for bad in ((-1, 1, 0), (9, 1, 0), (3, 2, 0), (3, -1, 0), (3, 1, 1)):
        assert fs.lib.fluid_sdf_set_track(h, C.byref(fs.SdfTrack(*bad))) == ERR_ARG, bad
    assert fs.lib.fluid_sdf_set_track(None, C.byref(fs.SdfTrack(3, 1, 0))) == ERR_ARG
    p1 = fs.water_cube_drop(n, 4, seed=0)
    sim.upload_particles(p1)
    sim.sdf_snapshot(R, w, smooth=(1, 1, 3.0))                                   # the refused settings left tracking off: |off| > bg is fine
    assert sim.sdf_wait().n_leaves > 0
    assert fs.lib.fluid_sdf_set_track(h, C.byref(fs.SdfTrack(8, 1, 0))) == 0 and fs.lib.fluid_sdf_set_track(h, C.byref(fs.SdfTrack(0, 0, 0))) == 0
    sim.sdf_set_track(3, True)
    bg = float(np.float32(w))
    far = fs.SdfFilter(1, 1, bg * 1.01)
    g = fs.SdfGridC()
    for f in (far, fs.SdfFilter(1, 0, -bg * 1.01)):
        assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(f)) == ERR_ARG
        assert "offset" in fs.lib.fluid_last_error().decode()
        assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(f)) == ERR_ARG
        assert fs.lib.fluid_sdf_snapshot_attr(h, C.byref(prm), C.byref(f)) == ERR_ARG
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE                     # none of the refused calls left a snapshot behind
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(fs.SdfFilter(1, 1, -bg))) == 0       # the limit itself
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == 0
    c1, c2 = (1, 1, -0.25, 3, 1), (2, 2, 0.0, 2, 1)
    sim.sdf_snapshot(R, w, smooth=args_of(c1, dx)[0])
    sim.mesh_snapshot(R, w, smooth=args_of(c1, dx)[0])
    sim.step()
    p2, _ = sim.download_particles()
    sim.sdf_set_track(2, True)
    sim.sdf_snapshot(R, w, smooth=args_of(c2, dx)[0])
    sim.mesh_snapshot(R, w, smooth=args_of(c2, dx)[0])
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE      # a third
    assert "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE
    ga, gb = sim.sdf_wait(), sim.sdf_wait()
    ma, mb = sim.mesh_wait(), sim.mesh_wait()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE
    l1, r1, _ = ref_of(p1, n, R, w, dx, c1)
    l2, r2, _ = ref_of(p2, n, R, w, dx, c2)
    for got, ref in ((ga, l1), (gb, l2)):
        assert np.array_equal(got.origin, ref[0]) and np.array_equal(u32(got.values), u32(ref[1])) and np.array_equal(got.active, ref[2])
    same_mesh(ma, r1[0], r1[1], "first")
    same_mesh(mb, r2[0], r2[1], "second")
    assert len(r1[0]) > 0
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    assert fs.lib.fluid_sdf_set_track(sim._h, C.byref(fs.SdfTrack(3, 1, 0))) == ERR_STATE
    assert "fluid_sdf_filter_tracked" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_set_track(sim._h, None) == ERR_STATE
    with pytest.raises(fs.FluidError):
        sim.sdf_set_track(3)
    sim.close()
    grp.close()


def test_tracked_snapshots_do_not_disturb_the_steps(fs):
    """The same input on two handles: B takes tracked surface and mesh snapshots after every step, A nothing.  Particles bit for
    bit and every field of the step stats as on A."""
    n, (R, w, dx) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=3)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    for s in (a, b):
        s.upload_particles(pos)
    b.sdf_set_track(3, True)
    sa, sb = [], []
    for k in range(5):
        sa.append(a.step())
        sb.append(b.step())
        filt = (1, 1 + (k & 1), -0.25)
        b.sdf_snapshot(R, w, smooth=filt)
        b.mesh_snapshot(R, w, smooth=filt)
        g = b.sdf_wait()
        v, q = b.mesh_wait()
        assert g.n_leaves > 0 and len(v) > 0 and len(q) > 0 and q.max() < len(v)
    assert sa == sb
    (pa, va), (pb, vb) = a.download_particles(), b.download_particles()
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    case = (1, 1, -0.25, 3, 1)
    leaves, mesh, _ = ref_of(pb, n, R, w, dx, case)                              # ... and the last snapshots' kind is the reference's
    check(fs, b, leaves, mesh, R, w, dx, case, "after 5 steps")
    for s in (a, b):
        s.close()


@pytest.mark.parametrize("dims", [(2, 1, 1), (2, 2, 2)])
def test_blocks_track_the_merged_list(fs, dims):
    """A decomposed run after 2 steps: the host tracked filter of the merged rank lists is the one-GPU handle's tracked snapshot of
    the same particles, and the host mesher of it is that handle's tracked mesh."""
    fd = fs.load_dist()
    n, (R, w, dx) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 4, seed=1)
    size = dims[0] * dims[1] * dims[2]
    grp = fd.LocalGroup(size)
    sims = [None] * size

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
    for case in ((1, 2, -0.25, 3, 1), (2, 1, 0.6, 2, 1)):
        filt, track = args_of(case, dx)
        host, kept = fs.sdf_filter_tracked(merged, filt, track)
        one.sdf_set_track(*track)
        one.sdf_snapshot(R, w, smooth=filt)
        g = one.sdf_wait()
        assert g.n_leaves > 8
        same_grid(host, g, f"blocks {dims} {case}")
        assert np.array_equal(merged.origin[kept], host.origin)
        hm = fs.sdf_mesh(host)
        one.mesh_snapshot(R, w, smooth=filt)
        v, q = one.mesh_wait()
        assert len(q) > 100
        same_mesh((hm.vertices, hm.quads), v, q, f"blocks {dims} {case}")
    leaves, mesh, _ = ref_of(allp, n, R, w, dx, (1, 2, -0.25, 3, 1))             # ... and both are the reference's
    check(fs, one, leaves, mesh, R, w, dx, (1, 2, -0.25, 3, 1))
    one.close()


def test_driver_writes_the_tracked_mesh(fs, tmp_path):
    """The `fluid` program with FLUID_OUT_MESH, FLUID_OUT_SMOOTH=1,2,-0.25 and FLUID_OUT_TRACK=3: mesh<i>.ply holds the handle's
    tracked mesh of the particles of step i times the voxel size; stdout and the other files are what they are without it."""
    import leaf_ref
    n, ppc, steps, (R, w, dx), case = 24, 4, 3, SETS[0], (1, 2, -0.25, 3, 1)
    smooth = run_fluid(tmp_path / "smooth", n, ppc, steps, FLUID_OUT_MESH=f"{R},{w}", FLUID_OUT_SMOOTH="1,2,-0.25")
    track = run_fluid(tmp_path / "track", n, ppc, steps, FLUID_OUT_MESH=f"{R},{w}", FLUID_OUT_SMOOTH="1,2,-0.25", FLUID_OUT_TRACK="3")
    assert smooth == track
    names = lambda m: sorted(str(p.relative_to(tmp_path / m)) for p in (tmp_path / m).rglob("*") if p.is_file())   # noqa: E731
    assert names("smooth") == names("track") and f"simulation/mesh{steps - 1}.ply" in names("track")
    for nm in names("smooth"):
        if not nm.endswith(".ply"):
            assert leaf_ref.same_file(tmp_path / "smooth" / nm, tmp_path / "track" / nm), nm
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    sim.sdf_set_track(3, True)
    for i in range(steps):
        sim.step()
        sim.mesh_snapshot(R, w, smooth=(1, 2, -0.25))
        v, q = sim.mesh_wait()
        fv, fq, _ = read_ply(tmp_path / "track" / f"simulation/mesh{i}.ply")
        assert len(q) > 0 and np.array_equal(u32(fv), u32(v * np.float32(dx))) and np.array_equal(fq, q), i
        pv, _, _ = read_ply(tmp_path / "smooth" / f"simulation/mesh{i}.ply")
        assert pv.shape != fv.shape or not np.array_equal(u32(pv), u32(fv))       # the tracking did something
    _, ref, _ = ref_of(sim.download_particles()[0], n, R, w, dx, case)           # ... and the last one is the reference's
    same_mesh((v, q), ref[0], ref[1])
    sim.close()


def test_driver_on_blocks_writes_the_tracked_mesh(fs, tmp_path):
    """FLUID_BLOCKS=2x1x1 with FLUID_BLOCKS_MESH, FLUID_OUT_SMOOTH=1,1,0.6 and FLUID_OUT_TRACK=2,1: mesh<i>.ply is the host mesher of
    the tracked merged list of the same run taken here (the program's cut planes, ids and upload), and the reference's; stdout
    is what it is without FLUID_OUT_TRACK."""
    fd = fs.load_dist()
    n, ppc, steps, (R, w, dx), case, dims = 24, 4, 2, SETS[0], (1, 1, 0.6, 2, 1), (2, 1, 1)
    plain = run_fluid(tmp_path / "plain", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_MESH=f"{R},{w}", FLUID_OUT_SMOOTH="1,1,0.6")
    track = run_fluid(tmp_path / "track", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_MESH=f"{R},{w}", FLUID_OUT_SMOOTH="1,1,0.6", FLUID_OUT_TRACK="2,1")
    assert plain == track
    pos = fs.water_cube_drop(n, ppc, seed=0)
    grp = fd.LocalGroup(2)
    sims = [None] * 2

    def run(r):
        sim = fd.DistFluidSim(n, dims, fd.partition_blocks(n, pos, dims), grp.comms[r])
        sims[r] = sim
        sim.upload_global(pos)
        out = []
        for _ in range(steps):
            sim.step()
            sim.sdf_snapshot(R, w)
            out.append((sim.sdf_wait(), sim.download_local()[0]))
        return out

    try:
        res = grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    filt, tr = args_of(case, dx)
    for i in range(steps):
        merged = fs.merge_sdf_grids([r[i][0] for r in res])
        host, _ = fs.sdf_filter_tracked(merged, filt, tr)
        hm = fs.sdf_mesh(host)
        fv, fq, _ = read_ply(tmp_path / "track" / f"simulation/mesh{i}.ply")
        assert len(hm.quads) > 0 and np.array_equal(u32(fv), u32(hm.vertices * np.float32(dx))) and np.array_equal(fq, hm.quads), i
        pv, _, _ = read_ply(tmp_path / "plain" / f"simulation/mesh{i}.ply")
        assert pv.shape != fv.shape or not np.array_equal(u32(pv), u32(fv))       # the tracking did something
        _, ref, _ = ref_of(np.concatenate([r[i][1] for r in res]), n, R, w, dx, case)
        same_mesh((hm.vertices, hm.quads), ref[0], ref[1], f"step {i}")


@pytest.mark.parametrize("extra", [{"FLUID_OUT_SMOOTH": ""}, {"FLUID_OUT_TRACK": "9"}, {"FLUID_OUT_TRACK": "3,2"}, {"FLUID_OUT_TRACK": "x"},
                                   {"FLUID_OUT_TRACK": "3,"}, {"FLUID_OUT_TRACK": "-1"},
                                   {"FLUID_OUT_MESH": "", "FLUID_BLOCKS": "2x1x1", "FLUID_BLOCKS_MESH": "1.5,2.5", "FLUID_BLOCKS_MESH_VEL": "1"}])
def test_driver_refuses_a_tracking_it_would_not_apply(fs, tmp_path, extra):
    """Without FLUID_OUT_SMOOTH, malformed or out of limits, or with FLUID_BLOCKS_MESH_VEL: refused before any handle is created."""
    env = fluid_env(tmp_path, 16, 1, 1, FLUID_OUT_MESH="1.5,2.5", FLUID_OUT_SMOOTH="1,1", FLUID_OUT_TRACK="3")
    env.update(extra)
    r = subprocess.run([os.path.join(ROOT, "fluid-simulation_amd", "fluid")], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and "FLUID_OUT_TRACK" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not list(tmp_path.rglob("*.ply")) and not list(tmp_path.rglob("*.vdb"))
