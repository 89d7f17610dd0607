"""GPU (-m gpu): the smoothed liquid surface (fluid_sdf_snapshot_filtered / fluid_mesh_snapshot_filtered, kernels_sdf_filter.hip).
In every comparison the device list equals tests/sdf_filter_ref.py of tests/sdf_ref.py closed() — origins, masks, values as bit
patterns — and the device mesh equals tests/mesh_ref.py of that filtered field: vertices as bit patterns, quads exactly."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref
import sdf_filter_ref
import sdf_ref
from sdf_testlib import read_ply, run_fluid, same_grid, u32

pytestmark = pytest.mark.gpu

SETS = mesh_ref.SETS
FILTERS = sdf_filter_ref.FILTERS
SCENES = ["one", "corner", "lo", "hi", "cloud"]
ERR_ARG, ERR_STATE = 1, 3
LEAF_BYTES = 2048 + 64 + 12


def same_mesh(got, vert, quads, what=""):
    v, q = got
    assert v.shape == vert.shape and q.shape == quads.shape, (what, v.shape, vert.shape, q.shape, quads.shape)
    assert v.dtype == np.float32 and q.dtype == np.uint32
    assert np.array_equal(u32(v), u32(vert)), what
    assert np.array_equal(q, quads), what


def ref_of(pos, n, R, w, dx, filt):
    """(leaf list (origin, values, active) of the filtered field, its mesh) from the numpy references."""
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    bg = sdf_ref.constants(R, w, dx)[3]
    vf = sdf_filter_ref.smooth(val, act, bg, *filt)
    return sdf_ref.leaf_list(vf, act, bg), mesh_ref.mesh(vf)


def check(fs, sim, leaves, mesh, R, w, filt, what=""):
    """The handle's filtered surface list is `leaves`, its filtered mesh is `mesh`; so are the host filter's and the host mesher's."""
    what = f"{what} {filt}"
    org, v, a = leaves
    sim.sdf_snapshot(R, w, smooth=filt)
    g = sim.sdf_wait()
    assert g.n_leaves == len(org) and np.array_equal(g.origin, org), what
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what
    assert sim.sdf_stats()["leaves_listed"] == len(org) and sim.sdf_stats()["bytes_to_host"] == len(org) * LEAF_BYTES + 4
    sim.mesh_snapshot(R, w, smooth=filt)
    got = sim.mesh_wait()
    same_mesh(got, mesh[0], mesh[1], what)
    assert sim.mesh_stats() == {"vertices": len(mesh[0]), "quads": len(mesh[1]), "bytes_to_host": 12 * len(mesh[0]) + 16 * len(mesh[1]) + 8}, what
    return g, got


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", SCENES)
def test_filtered_surface_and_mesh_are_the_reference(fs, name, n, R, w, dx):
    """Odd pass counts (K = 1, 3: the result ends in the second buffer) and even ones (K = 2: in the first), the offset alone
    (K = 0) and the identity."""
    sim = fs.FluidSim(n=n, dx=dx)
    pos = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))[0]
    sim.upload_particles(pos)
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    sim.mesh_snapshot(R, w)
    plain_mesh = sim.mesh_wait()
    assert plain.n_leaves > 0
    for filt in FILTERS:
        _, vf, act, bg, mesh = sdf_filter_ref.scene(name, n, R, w, dx, filt)
        g, got = check(fs, sim, sdf_ref.leaf_list(vf, act, bg), mesh, R, w, filt, name)
        same_grid(g, fs.sdf_filter(plain, *filt), f"host filter {filt}")
        if filt == (1, 0, 0.0):                                                  # the unfiltered snapshot's bytes
            same_grid(g, plain, "identity")
            same_mesh(got, plain_mesh[0], plain_mesh[1], "identity")
        if (name, n, R, w) == ("cloud", 25, 3.0, 1.0) and filt[2] == 0.0 and filt[1] > 0:
            assert 2448 <= len(got[0]) <= 2871, (filt, len(got[0]))
        if (name, R, w, filt) == ("lo", 1.5, 2.5, (1, 2, 0.0)):                  # smoothed away: an EMPTY mesh while leaves are listed
            assert len(got[0]) == 0 and len(got[1]) == 0 and g.n_leaves > 0 and len(plain_mesh[0]) > 0
    sim.close()


@pytest.mark.parametrize("filt", [(1, 0, -0.9), (1, 1, -0.9)])
def test_mesh_range_is_the_box_dilated_by_five(fs, filt):
    """One particle whose base cell is -4 on every axis, R = 3, w = 1, grown by 0.9: inside voxels reach -8 and vertices the cells
    with min corner -9, in the leaf at -16 — one leaf below the range of the unfiltered mesh."""
    n, (R, w, dx) = 32, (3.0, 1.0, 1.0)
    pos = np.array([[-4.49, -4.49, -4.49]])
    leaves, mesh = ref_of(pos, n, R, w, dx, filt)
    assert (len(mesh[0]), len(mesh[1])) == (314, 312) and mesh[2].min() == -9 and (mesh[2] & ~7).min() == -16
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    check(fs, sim, leaves, mesh, R, w, filt)
    sim.mesh_snapshot(R, w)                                                      # the unfiltered one keeps its range and its bytes
    m0 = mesh_ref.mesh(sdf_ref.closed(pos, n, R, w, dx)[0])
    same_mesh(sim.mesh_wait(), m0[0], m0[1], "unfiltered")
    sim.close()


def test_cloud_and_stale_scratch(fs):
    """The cloud with (1, 1, 0) writes both buffers; then, on the same handle, single particles far from where the cloud's listed
    leaves were, with K = 1 and K = 2: the leaves of the new range that no particle reaches keep the cloud's values and masks in
    BOTH buffers — neither the passes nor what follows may read them.  Then the cloud again."""
    n, (R, w, dx) = 25, (1.0, 1.0, 1.0)
    pos = mesh_ref.positions("cloud", n)
    cl, cm = ref_of(pos, n, R, w, dx, (1, 1, 0.0))
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    check(fs, sim, cl, cm, R, w, (1, 1, 0.0), "cloud")
    for p in ([[10.3, 10.2, -9.6]], [[-10.4, 9.7, 10.1]], [[0.3, -0.2, 0.41]], [[10.3, 10.2, -9.6], [-10.4, -9.7, 10.1]]):
        one = np.array(p)
        for filt in ((1, 1, 0.0), (1, 2, 0.0)):
            sim.upload_particles(one)
            l1, m1 = ref_of(one, n, R, w, dx, filt)
            assert 0 < len(l1[0]) < 30
            check(fs, sim, l1, m1, R, w, filt, f"particles {p} after the cloud")
            sim.upload_particles(pos)
            check(fs, sim, cl, cm, R, w, (1, 1, 0.0), "cloud again")
    sim.close()


def test_slots_and_refusals(fs):
    n, (R, w, dx) = 32, SETS[0]
    sim = fs.FluidSim(n=n)
    h = sim._h
    prm = fs.SdfParams(R, w)
    ok = fs.SdfFilter(1, 1, 0.0)
    for bad in ((0, 1, 0.0), (5, 1, 0.0), (1, -1, 0.0), (1, 17, 0.0), (1, 1, float("nan")), (1, 1, float("inf"))):
        assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(fs.SdfFilter(*bad))) == ERR_ARG, bad
        assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(fs.SdfFilter(*bad))) == ERR_ARG, bad
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), None) == ERR_ARG and fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), None) == ERR_ARG
    assert fs.lib.fluid_sdf_snapshot_filtered(h, None, C.byref(ok)) == ERR_ARG and fs.lib.fluid_mesh_snapshot_filtered(h, None, C.byref(ok)) == ERR_ARG
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(fs.SdfParams(2.0, 2.5)), C.byref(ok)) == ERR_ARG
    g = fs.SdfGridC()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE                     # none of the refused calls left a snapshot behind
    sim.sdf_snapshot(R, w, smooth=(2, 1))                                        # no particles at all: an empty list
    assert sim.sdf_wait().n_leaves == 0
    p1 = fs.water_cube_drop(n, 4, seed=0)
    sim.upload_particles(p1)
    f1, f2 = (1, 1, -0.25), (2, 2, 0.0)
    sim.sdf_snapshot(R, w, smooth=f1)                                            # filtered and unfiltered share the two slots
    sim.mesh_snapshot(R, w, smooth=f1)
    sim.step()
    p2, _ = sim.download_particles()
    sim.sdf_snapshot(R, w)
    sim.mesh_snapshot(R, w, smooth=f2)
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE      # a third
    assert "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_snapshot(h, C.byref(prm)) == ERR_STATE
    assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE
    assert "two mesh snapshots" in fs.lib.fluid_last_error().decode()
    g1, g2, m1, m2 = fs.SdfGridC(), fs.SdfGridC(), fs.MeshC(), fs.MeshC()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g1)) == 0 and fs.lib.fluid_sdf_wait(h, C.byref(g2)) == 0
    assert fs.lib.fluid_mesh_wait(h, C.byref(m1)) == 0 and fs.lib.fluid_mesh_wait(h, C.byref(m2)) == 0
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE

    def gview(gc):
        k = gc.n_leaves
        org = np.ctypeslib.as_array(C.cast(gc.origin, C.POINTER(C.c_int32)), shape=(k, 3))
        val = np.ctypeslib.as_array(C.cast(gc.values, C.POINTER(C.c_float)), shape=(k, 512))
        wrd = np.ctypeslib.as_array(C.cast(gc.active, C.POINTER(C.c_uint64)), shape=(k, 8))
        return org, val, np.unpackbits(wrd.view(np.uint8), axis=1, bitorder="little").astype(bool)

    def mview(mc):
        v = np.ctypeslib.as_array(C.cast(mc.vertices, C.POINTER(C.c_float)), shape=(mc.n_vertices, 3))
        q = np.ctypeslib.as_array(C.cast(mc.quads, C.POINTER(C.c_uint32)), shape=(mc.n_quads, 4))
        return v, q
    # the first one's pointers are intact after the second snapshot and both waits
    l1, r1 = ref_of(p1, n, R, w, dx, f1)
    l2, _ = ref_of(p2, n, R, w, dx, (1, 0, 0.0))
    _, r2 = ref_of(p2, n, R, w, dx, f2)
    for gc, ref in ((g1, l1), (g2, l2)):
        org, val, act = gview(gc)
        assert np.array_equal(org, ref[0]) and np.array_equal(u32(val), u32(ref[1])) and np.array_equal(act, ref[2])
    same_mesh(mview(m1), r1[0], r1[1], "first")
    same_mesh(mview(m2), r2[0], r2[1], "second")
    assert len(r1[0]) > 0 and len(r2[0]) > 0 and not np.array_equal(u32(l1[1]), u32(ref_of(p1, n, R, w, dx, (1, 0, 0.0))[0][1]))
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    h = sim._h
    prm, ok = fs.SdfParams(1.5, 2.5), fs.SdfFilter(1, 1, 0.0)
    assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE
    assert "fluid_sdf_filter" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(ok)) == ERR_STATE
    assert "fluid_sdf_filter" in fs.lib.fluid_last_error().decode()
    sim.close()
    grp.close()


def test_filtered_snapshots_do_not_disturb_the_steps(fs):
    """The same input on two handles: B takes filtered surface and mesh snapshots after every step, A nothing.  Particles bit for
    bit and every field of the step stats as on A."""
    n, (R, w, _) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=3)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    for s in (a, b):
        s.upload_particles(pos)
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
    leaves, mesh = ref_of(pb, n, R, w, 1.0, (1, 1, -0.25))                       # ... and the last snapshots' kind is the reference's
    check(fs, b, leaves, mesh, R, w, (1, 1, -0.25), "after 5 steps")
    for s in (a, b):
        s.close()


@pytest.mark.parametrize("dims", [(2, 1, 1), (2, 2, 2)])
def test_blocks_filter_the_merged_list(fs, dims):
    """A decomposed run after 2 steps: the host filter of the merged rank lists is the one-GPU handle's filtered snapshot of the same
    particles, and the host mesher of it is that handle's filtered mesh."""
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
    for filt in ((1, 2, -0.25), (2, 1, 0.0)):
        host = fs.sdf_filter(merged, *filt)
        one.sdf_snapshot(R, w, smooth=filt)
        g = one.sdf_wait()
        assert g.n_leaves > 8
        same_grid(host, g, f"blocks {dims} {filt}")
        hm = fs.sdf_mesh(host)
        one.mesh_snapshot(R, w, smooth=filt)
        v, q = one.mesh_wait()
        assert len(q) > 100
        same_mesh((hm.vertices, hm.quads), v, q, f"blocks {dims} {filt}")
    leaves, mesh = ref_of(allp, n, R, w, dx, (1, 2, -0.25))                      # ... and both are the reference's
    check(fs, one, leaves, mesh, R, w, (1, 2, -0.25))
    one.close()


def test_driver_writes_the_smoothed_mesh(fs, tmp_path):
    """The `fluid` program with FLUID_OUT_MESH and FLUID_OUT_SMOOTH=1,2,-0.25: mesh<i>.ply holds the handle's filtered mesh of the
    particles of step i times the voxel size; stdout and the other files are what they are without FLUID_OUT_SMOOTH."""
    import leaf_ref
    n, ppc, steps, (R, w, dx), filt = 24, 4, 3, SETS[0], (1, 2, -0.25)
    plain = run_fluid(tmp_path / "plain", n, ppc, steps, FLUID_OUT_MESH=f"{R},{w}")
    smooth = run_fluid(tmp_path / "smooth", n, ppc, steps, FLUID_OUT_MESH=f"{R},{w}", FLUID_OUT_SMOOTH="1,2,-0.25")
    assert plain == smooth
    names = lambda m: sorted(str(p.relative_to(tmp_path / m)) for p in (tmp_path / m).rglob("*") if p.is_file())   # noqa: E731
    assert names("plain") == names("smooth") and f"simulation/mesh{steps - 1}.ply" in names("smooth")
    for nm in names("plain"):
        if not nm.endswith(".ply"):
            assert leaf_ref.same_file(tmp_path / "plain" / nm, tmp_path / "smooth" / nm), nm
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    for i in range(steps):
        sim.step()
        sim.mesh_snapshot(R, w, smooth=filt)
        v, q = sim.mesh_wait()
        fv, fq, _ = read_ply(tmp_path / "smooth" / f"simulation/mesh{i}.ply")
        assert len(q) > 0 and np.array_equal(u32(fv), u32(v * np.float32(dx))) and np.array_equal(fq, q), i
        pv, _, _ = read_ply(tmp_path / "plain" / f"simulation/mesh{i}.ply")
        assert pv.shape != fv.shape or not np.array_equal(u32(pv), u32(fv))       # the smoothing did something
    _, ref = ref_of(sim.download_particles()[0], n, R, w, dx, filt)              # ... and the last one is the reference's
    same_mesh((v, q), ref[0], ref[1])
    sim.close()


def test_driver_on_blocks_writes_the_smoothed_surface(fs, tmp_path):
    """FLUID_BLOCKS=2x1x1 with FLUID_BLOCKS_SURFACE and FLUID_OUT_SMOOTH: surface<i>.vdb, re-read by tests/vdb_reader.py, is the
    filtered level set of the blocks' particles; stdout and the density files are what they are without FLUID_OUT_SMOOTH."""
    import leaf_ref
    import vdb_reader
    fd = fs.load_dist()
    n, ppc, steps, (R, w, dx), filt, dims = 24, 4, 3, SETS[0], (1, 2, -0.25), (2, 1, 1)
    lo, hi, _, _ = sdf_ref.geometry(n)
    plain = run_fluid(tmp_path / "plain", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_SURFACE=f"{R},{w}")
    smooth = run_fluid(tmp_path / "smooth", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_SURFACE=f"{R},{w}", FLUID_OUT_SMOOTH="1,2,-0.25")
    assert plain == smooth
    for nm in ["mygrids.vdb"] + [f"simulation/mygrids{i}.vdb" for i in range(steps)]:
        assert leaf_ref.same_file(tmp_path / "plain" / nm, tmp_path / "smooth" / nm), nm
    # the same run here: the program's cut planes, ids and upload
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
            out.append(sim.download_local()[0])
        return out

    try:
        res = grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        val, act = sdf_ref.closed(np.concatenate([r[i] for r in res]), n, R, w, dx)
        vf = sdf_filter_ref.smooth(val, act, bg, *filt)
        _, grids = vdb_reader.read(tmp_path / "smooth" / f"simulation/surface{i}.vdb")
        assert len(grids) == 1 and grids[0].name == "surface" and np.float32(grids[0].background) == bg
        rv, ra = grids[0].dense(lo, hi)
        assert act.any() and np.array_equal(ra, act) and np.array_equal(u32(rv), u32(vf)), i
        assert not np.array_equal(u32(vf), u32(val))
        assert sorted(grids[0].leaves) == [tuple(o) for o in sdf_ref.leaf_list(vf, act, bg)[0].tolist()]
