"""GPU (-m gpu): the flows of the liquid surface (fluid_sdf_set_filter_kind, kernels_sdf_flow.hip).  In every comparison the device
list equals tests/sdf_flow_ref.py — a reference that knows no leaves and no range — in origins, masks and values as bit patterns,
and equals the host function's (fluid_sdf_flow) of the unfiltered list; once per kind the attribute snapshot, the filtered mesh and
a rendered image are checked against the matching references."""
import ctypes as C

import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_flow_ref as R
import sdf_ref
from sdf_testlib import run_fluid, same_grid, u32

pytestmark = pytest.mark.gpu

SET = (2.0, 2.0, 1.0)                                     # R, w, dx
FORMS = [("untracked", 0, False, False), ("tracked", 3, True, False), ("grown", 3, True, True)]   # name, N, trim, grow
ERR_ARG, ERR_STATE = 1, 3


def is_dense(g, dense, bg, what=""):
    org, v, a = sdf_ref.leaf_list(dense[0], dense[1], bg)
    assert g.n_leaves == len(org) and np.array_equal(g.origin, org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what
    return org


def start(fs, name, n, Rad, w, dx):
    pos = R.base(name, n, Rad, w, dx)[0]
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, attr_ref.velocities(pos))
    sim.sdf_snapshot(Rad, w, attr=True)
    plain, plain_attr = sim.sdf_wait_attr()
    assert plain.n_leaves > 0
    return sim, plain, plain_attr


def set_form(sim, N, trim, grow):
    sim.sdf_set_track(N if (N or trim) else None, trim, grow=grow)


@pytest.mark.parametrize("kind,W", R.CASES)
@pytest.mark.parametrize("name,n", R.SCENES)
def test_flow_is_the_reference_and_the_host_function(fs, name, n, kind, W):
    """K = 1 and K = 2 (the result ends in either buffer; K = 2 with an offset), untracked, tracked and grown, on one handle."""
    Rad, w, dx = SET
    sim, plain, _ = start(fs, name, n, Rad, w, dx)
    bg = R.base(name, n, Rad, w, dx)[5]
    sim.sdf_set_filter_kind(kind)
    for form, N, trim, grow in FORMS:
        set_form(sim, N, trim, grow)
        for K, units in ((1, 0.0), (2, -0.6 if grow else 0.6)):
            what = f"{name} {n} {R.NAMES[kind]} W={W} {form} K={K}"
            sim.sdf_snapshot(Rad, w, smooth=(W, K, units * dx))
            g = sim.sdf_wait()
            is_dense(g, R.scene(name, n, Rad, w, dx, kind, W, K, units, N, trim, grow), bg, what)
            same_grid(g, fs.sdf_flow(plain, kind, (W, K, units * dx), track=(N, trim) if N else None, grow=grow), what + " (host function)")
    sim.close()


@pytest.mark.parametrize("Rad,w,dx", [(1.0, 2.0, 0.5)])
@pytest.mark.parametrize("kind,W", R.CASES)
def test_another_voxel_size(fs, kind, W, Rad, w, dx):
    name, n = "leafcorner", 32
    sim, plain, _ = start(fs, name, n, Rad, w, dx)
    bg = R.base(name, n, Rad, w, dx)[5]
    sim.sdf_set_filter_kind(kind)
    for form, N, trim, grow in FORMS:
        set_form(sim, N, trim, grow)
        sim.sdf_snapshot(Rad, w, smooth=(W, 2, 0.0))
        is_dense(sim.sdf_wait(), R.scene(name, n, Rad, w, dx, kind, W, 2, 0.0, N, trim, grow), bg, f"{R.NAMES[kind]} {form}")
    sim.close()


@pytest.mark.parametrize("kind,W", R.CASES)
def test_attributes_mesh_and_image_of_the_cloud(fs, kind, W):
    """Once per kind, tracked and grown (K = 2): the attribute snapshot (ids and velocities of the voxels still active untouched, those
    of the reference), the filtered mesh (mesh_ref of the reference field, fluid_sdf_mesh of the host list) and one image
    (fluid_sdf_render of the list)."""
    name, n, (Rad, w, dx) = "cloud", 16, SET
    sim, plain, plain_attr = start(fs, name, n, Rad, w, dx)
    bg = R.base(name, n, Rad, w, dx)[5]
    sim.sdf_set_filter_kind(kind)
    filt = (W, 2, 0.0)
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=48, height=32)
    for form, N, trim, grow in FORMS:
        what = f"{R.NAMES[kind]} W={W} {form}"
        set_form(sim, N, trim, grow)
        dense = R.scene(name, n, Rad, w, dx, kind, W, 2, 0.0, N, trim, grow)
        sim.sdf_snapshot(Rad, w, smooth=filt, attr=True)
        g, at = sim.sdf_wait_attr()
        org = is_dense(g, dense, bg, what)
        li, lv = attr_ref.leaf_attr(dense[2], dense[3], org)
        assert np.array_equal(at.id, li) and np.array_equal(u32(at.velocity), u32(lv)), what
        host, hat = fs.sdf_flow(plain, kind, filt, track=(N, trim) if N else None, grow=grow, attr=plain_attr)
        same_grid(g, host, what + " (host function)")
        assert np.array_equal(at.id, hat.id) and np.array_equal(u32(at.velocity), u32(hat.velocity)), what
        if not grow:                                                          # untouched: what the unfiltered snapshot gave, where still active
            was = {tuple(o): i for i, o in enumerate(plain.origin)}
            for i, o in enumerate(g.origin):
                k, a = was[tuple(o)], g.active[i]
                assert np.array_equal(at.id[i][a], plain_attr.id[k][a]) and np.array_equal(u32(at.velocity[i][:, a]), u32(plain_attr.velocity[k][:, a])), what
        ref = mesh_ref.mesh(dense[0])
        sim.mesh_snapshot(Rad, w, smooth=filt)
        mv, mq = sim.mesh_wait()[:2]
        assert len(ref[0]) > 0 and mv.shape == ref[0].shape and np.array_equal(u32(mv), u32(ref[0])) and np.array_equal(mq, ref[1]), what
        hm = fs.sdf_mesh(host)
        assert np.array_equal(u32(mv), u32(hm.vertices)) and np.array_equal(mq, hm.quads), what
        sim.render_snapshot(Rad, w, cam, smooth=filt, depth=True, normals=True)
        img = sim.render_wait()
        himg = fs.sdf_render(g, cam, None, True, True, True)
        assert img["n_hit"] == himg["n_hit"] > 0, what
        assert np.array_equal(img["rgb"], himg["rgb"]) and np.array_equal(u32(img["depth"]), u32(himg["depth"])), what
        assert np.array_equal(u32(img["normals"]), u32(himg["normals"])), what
    sim.close()


def test_kind_box_gives_the_box_filter_again_and_the_errors(fs):
    name, n, (Rad, w, dx) = "cloud", 16, SET
    sim, plain, _ = start(fs, name, n, Rad, w, dx)
    h = sim._h
    filt = (2, 2, 0.5)
    sim.sdf_snapshot(Rad, w, smooth=filt)
    before = sim.sdf_wait()
    same_grid(before, fs.sdf_filter(plain, *filt), "the box filter before any setting")
    sim.sdf_set_track(3, True)
    sim.sdf_snapshot(Rad, w, smooth=filt)
    tracked_before = sim.sdf_wait()
    for kind, W in R.CASES:
        sim.sdf_set_filter_kind(kind)
        sim.sdf_set_track(None)
        sim.sdf_snapshot(Rad, w, smooth=(W, 2, 0.5))
        assert not np.array_equal(u32(sim.sdf_wait().values), u32(before.values)), kind
        sim.sdf_set_filter_kind("box")
        sim.sdf_snapshot(Rad, w, smooth=filt)
        same_grid(sim.sdf_wait(), before, f"box after {R.NAMES[kind]}")
        sim.sdf_set_track(3, True)
        sim.sdf_snapshot(Rad, w, smooth=filt)
        same_grid(sim.sdf_wait(), tracked_before, f"tracked box after {R.NAMES[kind]}")
    sim.sdf_set_track(None)
    # a bad kind is refused and leaves the setting as it was
    for bad in (-1, 4, 256):
        assert fs.lib.fluid_sdf_set_filter_kind(h, bad) == ERR_ARG, bad
    assert fs.lib.fluid_sdf_set_filter_kind(None, 1) == ERR_ARG
    with pytest.raises(fs.FluidError) as e:
        sim.sdf_set_filter_kind(7)
    assert e.value.code == ERR_ARG
    sim.sdf_snapshot(Rad, w, smooth=filt)
    same_grid(sim.sdf_wait(), before, "box after a refused kind")
    # the width rule of a kind: checked where a filtered snapshot begins, by every entry point that takes a filter
    prm, g = fs.SdfParams(Rad, w), fs.SdfGridC()
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=16, height=8)
    for kind, W in [(R.CURVATURE, 2), (R.LAPLACIAN, 2), (R.MEDIAN, 3), (R.CURVATURE, 4)]:
        sim.sdf_set_filter_kind(kind)
        f = fs.SdfFilter(W, 1, 0.0)
        assert fs.lib.fluid_sdf_snapshot_filtered(h, C.byref(prm), C.byref(f)) == ERR_ARG, (kind, W)
        assert "fluid_sdf_set_filter_kind" in fs.lib.fluid_last_error().decode()
        assert fs.lib.fluid_mesh_snapshot_filtered(h, C.byref(prm), C.byref(f)) == ERR_ARG
        assert fs.lib.fluid_sdf_snapshot_attr(h, C.byref(prm), C.byref(f)) == ERR_ARG
        assert fs.lib.fluid_mesh_snapshot_attr(h, C.byref(prm), C.byref(f)) == ERR_ARG
        assert fs.lib.fluid_mesh_snapshot_ex(h, C.byref(prm), C.byref(f), 2) == ERR_ARG
        assert fs.lib.fluid_render_snapshot(h, C.byref(prm), C.byref(f), C.byref(cam), None, 1) == ERR_ARG
        assert fs.lib.fluid_sdf_snapshot(h, C.byref(prm)) == 0                   # an unfiltered snapshot is untouched
        assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == 0 and g.n_leaves == plain.n_leaves
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE                     # none of the refused calls left a snapshot behind
    sim.sdf_set_filter_kind("box")
    sim.sdf_snapshot(Rad, w, smooth=(4, 1, 0.0))                                 # the box filter keeps its widths
    assert sim.sdf_wait().n_leaves > 0
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    for v in (R.MEDIAN, R.BOX):
        assert fs.lib.fluid_sdf_set_filter_kind(sim._h, v) == ERR_STATE
        assert "fluid_sdf_flow" in fs.lib.fluid_last_error().decode()
    sim.close()
    grp.close()


def test_driver_writes_the_curvature_flow_on_one_gpu_and_on_blocks(fs, tmp_path):
    """The `fluid` program with FLUID_OUT_SMOOTH=1,2, FLUID_OUT_TRACK=3,1,1 and FLUID_OUT_SMOOTH_KIND=curvature.  One GPU:
    surface<i>.vdb, re-read by tests/vdb_reader.py, is the handle's grown curvature flow of step i.  FLUID_BLOCKS=2x1x1: the file is
    fluid_sdf_flow of the unfiltered surface the same run writes without the variables (the writer-thread path)."""
    import vdb_reader
    n, ppc, steps, (Rad, w, dx) = 24, 4, 2, SET
    lo, hi, _, _ = sdf_ref.geometry(n)
    bg = sdf_ref.constants(Rad, w, dx)[3]
    flow = dict(FLUID_OUT_SMOOTH="1,2", FLUID_OUT_TRACK="3,1,1", FLUID_OUT_SMOOTH_KIND="curvature")
    plain = run_fluid(tmp_path / "plain", n, ppc, steps, FLUID_OUT_SURFACE=f"{Rad},{w}", FLUID_OUT_SMOOTH="1,2", FLUID_OUT_TRACK="3,1,1")
    one = run_fluid(tmp_path / "one", n, ppc, steps, FLUID_OUT_SURFACE=f"{Rad},{w}", **flow)
    assert plain == one                                                          # stdout is what it is without the variable
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    sim.sdf_set_track(3, True, grow=True)
    sim.sdf_set_filter_kind("curvature")
    for i in range(steps):
        sim.step()
        sim.sdf_snapshot(Rad, w, smooth=(1, 2, 0.0))
        g = sim.sdf_wait()
        _, grids = vdb_reader.read(tmp_path / "one" / f"simulation/surface{i}.vdb")
        assert len(grids) == 1 and grids[0].name == "surface" and np.float32(grids[0].background) == bg
        rv, ra = grids[0].dense(lo, hi)
        dv, da = fs.sdf_to_dense(g)
        assert g.n_leaves > 0 and np.array_equal(ra, da) and np.array_equal(u32(rv), u32(dv)), i
        _, boxed = vdb_reader.read(tmp_path / "plain" / f"simulation/surface{i}.vdb")
        assert not np.array_equal(u32(boxed[0].dense(lo, hi)[0]), u32(rv)), i      # the kind did something to the file
    sim.close()
    run_fluid(tmp_path / "raw", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_SURFACE=f"{Rad},{w}")
    run_fluid(tmp_path / "blocks", n, ppc, steps, FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_SURFACE=f"{Rad},{w}", **flow)
    fR, fw = sdf_ref.constants(Rad, w, dx)[:2]
    for i in range(steps):
        _, raw = vdb_reader.read(tmp_path / "raw" / f"simulation/surface{i}.vdb")
        val, act = raw[0].dense(lo, hi)
        org, v, a = sdf_ref.leaf_list(val, act, bg)
        host = fs.sdf_flow(fs.SdfGrid(n, org, v, a, bg, fR, fw), "curvature", (1, 2, 0.0), track=3, grow=True)
        _, grids = vdb_reader.read(tmp_path / "blocks" / f"simulation/surface{i}.vdb")
        rv, ra = grids[0].dense(lo, hi)
        hv, ha = fs.sdf_to_dense(host)
        assert host.n_leaves > 0 and np.array_equal(ra, ha) and np.array_equal(u32(rv), u32(hv)), i
