"""GPU (-m gpu): the HJWENO5 renormalisation of the liquid surface (fluid_sdf_set_track with scheme FLUID_SDF_TRACK_HJWENO5,
kernels_sdf_weno.hip).  In every comparison the device list equals tests/sdf_weno_ref.py of tests/sdf_ref.py closed() — origins,
masks, values as bit patterns — and the host function's (fluid_sdf_filter_tracked / _grown / fluid_sdf_flow with the same scheme);
the device mesh equals tests/mesh_ref.py of the tracked field and fluid_sdf_mesh of the tracked list: vertices as bit patterns,
quads exactly."""
import ctypes as C

import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_filter_ref
import sdf_flow_ref
import sdf_grow_ref
import sdf_ref
import sdf_weno_ref as W
from sdf_testlib import same_grid, same_mesh, u32

pytestmark = pytest.mark.gpu

SETS = mesh_ref.SETS
SCENES = ["one", "corner", "lo", "hi", "cloud"]
ERR_ARG, ERR_STATE = 1, 3
LEAF_BYTES = 2048 + 64 + 12
NO_ID = 0xFFFFFFFF
HJ = W.HJWENO5


def same_leaves(g, leaves, what=""):
    org, v, a = leaves
    assert g.n_leaves == len(org) and np.array_equal(g.origin, org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", SCENES)
def test_tracked_surface_and_mesh_are_the_reference(fs, name, n, R, w, dx):
    """Every case of CASES on one handle, one after the other; n = 16: two leaves per axis, both halo sides; n = 25: a last leaf
    that sticks out of the grid and range edges at both ends."""
    sim = fs.FluidSim(n=n, dx=dx)
    pos = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))[0]
    sim.upload_particles(pos)
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    assert plain.n_leaves > 0
    for case in W.CASES:
        Wd, K, units, N, tr = case
        what = f"{name} {n} {case}"
        vt, at, bg, mesh = W.scene(name, n, R, w, dx, case)
        filt = (Wd, K, units * dx)
        sim.sdf_set_track(N, bool(tr), scheme="hjweno5")
        sim.sdf_snapshot(R, w, smooth=filt)
        g = sim.sdf_wait()
        leaves = sdf_ref.leaf_list(vt, at, bg)
        same_leaves(g, leaves, what)
        st = sim.sdf_stats()
        assert st["leaves_listed"] == len(leaves[0]) and st["bytes_to_host"] == len(leaves[0]) * LEAF_BYTES + 4, what
        sim.mesh_snapshot(R, w, smooth=filt)
        got = sim.mesh_wait()
        same_mesh(got, mesh[0], mesh[1], what)
        host, _ = fs.sdf_filter_tracked(plain, filt, (N, bool(tr), HJ))
        same_grid(g, host, what + " (host function)")
        hm = fs.sdf_mesh(host)
        same_mesh(got, hm.vertices, hm.quads, what + " (host mesher)")
    sim.sdf_snapshot(R, w)                                                       # unfiltered snapshots are untouched by the setting
    same_grid(sim.sdf_wait(), plain, "unfiltered with tracking set")
    sim.close()


def test_grown_tracks_with_an_offset_and_attributes(fs):
    """grow=True with a tracked offset of 1.5 dx (three steps, three grown tracks), with attributes: the reference's and the host
    function's; and attr=True without growing: ids and velocities of trimmed voxels cleared, the rest untouched."""
    name, n, (R, w, dx) = "cloud", 25, SETS[3]
    pos, vel, val, act, ids, v32, bg = sdf_grow_ref.base(name, n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    sim.sdf_snapshot(R, w, attr=True)
    plain, plain_attr = sim.sdf_wait_attr()
    filt = (1, 1, -1.5 * dx)
    sim.sdf_set_track(3, True, grow=True, scheme="hjweno5")
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g, a = sim.sdf_wait_attr()
    vt, at, it, velt = W.grown(val, act, bg, dx, 1, 1, -1.5 * dx, 3, ids, v32)
    leaves = sdf_ref.leaf_list(vt, at, bg)
    same_leaves(g, leaves, "grown")
    assert g.n_leaves > plain.n_leaves                                           # the band walked outwards into unlisted leaves
    li, lv = attr_ref.leaf_attr(it, velt, leaves[0])
    assert np.array_equal(a.id, li) and np.array_equal(u32(a.velocity), u32(lv))
    host, hat = fs.sdf_filter_grown(plain, filt, (3, True, HJ), attr=plain_attr)
    same_grid(g, host, "grown (host function)")
    assert np.array_equal(a.id, hat.id) and np.array_equal(u32(a.velocity), u32(hat.velocity))
    sim.mesh_snapshot(R, w, smooth=filt)
    ref = mesh_ref.mesh(vt)
    same_mesh(sim.mesh_wait(), ref[0], ref[1], "grown mesh")
    first = sdf_grow_ref.grown(val, act, bg, dx, 1, 1, -1.5 * dx, 3)
    assert not np.array_equal(u32(first[0]), u32(vt))                            # the scheme did something
    # attributes without growing: the trim clears what it deactivates and nothing else
    filt = (1, 1, 0.0)
    sim.sdf_set_track(None)
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g0, a0 = sim.sdf_wait_attr()
    sim.sdf_set_track(3, True, scheme="hjweno5")
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g1, a1 = sim.sdf_wait_attr()
    vt, at = W.tracked(val, act, bg, dx, 1, 1, 0.0, 3, True)
    same_leaves(g1, sdf_ref.leaf_list(vt, at, bg), "attr")
    host, kept = fs.sdf_filter_tracked(plain, filt, (3, True, HJ))
    same_grid(g1, host, "attr (host function)")
    gone = g0.active[kept] & ~g1.active
    assert gone.sum() > 50 and not (g1.active & ~g0.active[kept]).any()
    assert (a1.id[gone] == NO_ID).all() and (a1.id[~g1.active] == NO_ID).all() and (a1.id[g1.active] != NO_ID).all()
    assert np.array_equal(a1.id[g1.active], a0.id[kept][g1.active])
    v1, v0 = a1.velocity.transpose(0, 2, 1), a0.velocity[kept].transpose(0, 2, 1)
    assert (u32(v1[~g1.active]) == 0).all()                                      # +0, not -0
    assert np.array_equal(u32(v1[g1.active]), u32(v0[g1.active]))
    sim.close()


def test_median_flow_tracked_with_the_scheme(fs):
    name, n, (R, w, dx) = "cloud", 16, SETS[3]
    _, _, val, act, _, _, bg = sdf_grow_ref.base(name, n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(sdf_grow_ref.positions(name, n))
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    sim.sdf_set_filter_kind("median")
    sim.sdf_set_track(3, True, scheme="hjweno5")
    filt = (1, 2, 0.6 * dx)
    sim.sdf_snapshot(R, w, smooth=filt)
    g = sim.sdf_wait()
    vt, at, _, _ = W.flow(sdf_flow_ref.MEDIAN, val, act, bg, dx, 1, 2, 0.6 * dx, 3, True, False)
    same_leaves(g, sdf_ref.leaf_list(vt, at, bg), "median")
    same_grid(g, fs.sdf_flow(plain, sdf_flow_ref.MEDIAN, filt, track=(3, True, HJ)), "median (host function)")
    sim.close()


def test_image_of_the_tracked_level_set(fs):
    """A 32 x 24 fluid_render_snapshot goes through the same front half: the image is fluid_sdf_render of the host-tracked list."""
    n, (R, w, dx) = 25, SETS[3]
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(mesh_ref.positions("cloud", n))
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    filt = (1, 1, 0.0)
    host, _ = fs.sdf_filter_tracked(plain, filt, (3, True, HJ))
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=32, height=24)
    sim.sdf_set_track(3, True, scheme="hjweno5")
    sim.render_snapshot(R, w, cam, smooth=filt, depth=True)
    img = sim.render_wait()
    ref = fs.sdf_render(host, cam, None, True, True, False)
    assert img["n_hit"] == ref["n_hit"] > 30
    assert np.array_equal(img["rgb"], ref["rgb"]) and np.array_equal(u32(img["depth"]), u32(ref["depth"]))
    sim.sdf_set_track(3, True)
    sim.render_snapshot(R, w, cam, smooth=filt, depth=True)
    assert not np.array_equal(u32(sim.render_wait()["depth"]), u32(img["depth"]))   # the scheme did something to the image
    sim.close()


def test_switching_the_scheme_and_the_refusals(fs):
    """first -> hjweno5 -> first on one handle: the first and the third snapshot are equal byte for byte, the second differs;
    unfiltered snapshots never change.  The ABI: scheme 4 accepted, -1, 1, 2, 3, 5 FLUID_ERR_ARG and the setting left as it was."""
    n, (R, w, dx) = 25, SETS[0]
    pos = mesh_ref.positions("cloud", n)
    sim = fs.FluidSim(n=n, dx=dx)
    h = sim._h
    sim.upload_particles(pos)
    filt = (1, 2, -0.25 * dx)
    sim.sdf_snapshot(R, w)
    plain = sim.sdf_wait()
    snaps, meshes = [], []
    for scheme in ("first", "hjweno5", 0):
        sim.sdf_set_track(3, True, scheme=scheme)
        sim.sdf_snapshot(R, w, smooth=filt)
        snaps.append(sim.sdf_wait())
        sim.mesh_snapshot(R, w, smooth=filt)
        meshes.append(sim.mesh_wait())
        sim.sdf_snapshot(R, w)
        same_grid(sim.sdf_wait(), plain, f"unfiltered under {scheme}")
    same_grid(snaps[0], snaps[2], "first again")
    same_mesh(meshes[0], meshes[2][0], meshes[2][1], "first again")
    assert snaps[0].n_leaves != snaps[1].n_leaves or not np.array_equal(u32(snaps[0].values), u32(snaps[1].values))
    assert fs.lib.fluid_sdf_set_track(h, C.byref(fs.SdfTrack(3, 1, HJ))) == 0
    for bad in (-1, 1, 2, 3, 5):
        assert fs.lib.fluid_sdf_set_track(h, C.byref(fs.SdfTrack(3, 1, bad))) == ERR_ARG, bad
        assert "FLUID_SDF_TRACK_HJWENO5" in fs.lib.fluid_last_error().decode()
        with pytest.raises(fs.FluidError):
            sim.sdf_set_track(3, True, scheme=bad)
    sim.sdf_snapshot(R, w, smooth=filt)                                          # the refused settings left scheme 4 standing
    same_grid(sim.sdf_wait(), snaps[1], "after the refusals")
    with pytest.raises(ValueError):
        sim.sdf_set_track(3, True, scheme="weno")
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    assert fs.lib.fluid_sdf_set_track(sim._h, C.byref(fs.SdfTrack(3, 1, HJ))) == ERR_STATE
    assert "fluid_sdf_filter_tracked" in fs.lib.fluid_last_error().decode()
    with pytest.raises(fs.FluidError):
        sim.sdf_set_track(3, scheme="hjweno5")
    sim.close()
    grp.close()
