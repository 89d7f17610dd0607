"""GPU (-m gpu): the averaged-position surface (fluid_sdf_set_surface, kernels_sdf_avg.hip) against tests/sdf_avg_ref.py: leaf
origins, masks and values (as bit patterns) must be equal exactly; what follows the search (filter, mesh, image) against the host
functions on the averaged list; the way back to the spheres; the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sdf_avg_ref
import sdf_ref
from sdf_avg_ref import block_and_scattered
from sdf_testlib import same_grid, same_mesh, u32
from test_gpu_sdf import check_grid

pytestmark = pytest.mark.gpu

SETS = [(1.0, 3.0, 1.0, 3.0), (1.5, 2.5, 1.0, 4.0), (3.0, 1.0, 1.0, 4.0), (1.0, 2.0, 0.5, 1.5)]      # (R, w, dx, h)
ERR_ARG, ERR_STATE = 1, 3


def check_avg(g, pos, n, R, w, dx, h, what=""):
    """g is exactly the leaf list of the reference's averaged grid for the particles `pos`.  Returns the reference (values, active)."""
    val, act = sdf_avg_ref.averaged(pos, n, R, w, dx, h)
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert g.n == n and (g.background, g.radius, g.half_width) == (bg, fR, fw), what
    assert g.n_leaves == len(org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.origin, org), what
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what
    return val, act


def snap(sim, R, w):
    sim.sdf_snapshot(R, w)
    return sim.sdf_wait()


@pytest.mark.parametrize("R,w,dx,h", SETS)
@pytest.mark.parametrize("n", [16, 25])
def test_one_particle(fs, n, R, w, dx, h):
    lo, hi, _, _ = sdf_ref.geometry(n)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.sdf_set_surface("averaged", h)
    cases = {"voxel centre": [1.0, -2.0, 3.0], "generic": [0.3, -1.7, 2.25], "round tie": [1.5, -2.5, 0.5],
             "wall cell at hi": [hi - 0.2, hi + 0.3, hi], "outside": [hi + 0.6, 0.0, 0.0]}
    for name, p in cases.items():
        pos = np.array([p])
        sim.upload_particles(pos)
        g = snap(sim, R, w)
        val, act = check_avg(g, pos, n, R, w, dx, h, name)
        assert (g.n_leaves == 0) == (name == "outside"), name
        if name != "outside":
            sval, sact = sdf_ref.closed(pos, n, R, w, dx)
            assert act.any() and np.array_equal(act, sact), name                  # one particle: a sphere
            assert np.abs(val.astype(np.float64) - sval).max() <= 1e-5 * dx, name
    sim.close()


def test_every_ring_reaches_the_sums(fs):
    """h = 4, voxel (0, 0, 0): a particle at (0.2, 0, 0), one at (3.9, 0.3, 0) — base cell 4, which must weigh — and one at
    (4, 0, 0), whose x2 is h2 exactly and weighs nothing; mirrored over the 6 permutations and the 8 signs."""
    n, (R, w, dx, h) = 16, SETS[1]
    lo = sdf_ref.geometry(n)[0]
    base = np.array([[0.2, 0.0, 0.0], [3.9, 0.3, 0.0], [4.0, 0.0, 0.0]])
    assert sdf_ref.base_cell(base).tolist() == [[0, 0, 0], [4, 0, 0], [4, 0, 0]]
    h2, ih2 = sdf_avg_ref.constants(h)
    x2 = sdf_ref.dist2(0, 0, 0, base)
    W = sdf_avg_ref.weight(x2, h2, ih2)
    assert x2[2] == h2 and W[2] == 0 and W[1] > 0 and W[0] > W[1]
    sim = fs.FluidSim(n=n)
    sim.sdf_set_surface("averaged", h)
    o = (-lo, -lo, -lo)
    for perm in itertools.permutations(range(3)):
        for sign in itertools.product((1.0, -1.0), repeat=3):
            pos = base[:, perm] * np.array(sign)
            sim.upload_particles(pos)
            g = snap(sim, R, w)
            val, act = check_avg(g, pos, n, R, w, dx, h, (perm, sign))
            SW = sdf_avg_ref.sums(pos, n, h)[1]
            assert SW[o] == W[0] + W[1] and act[o]
            without = sdf_avg_ref.averaged(pos[[0, 2]], n, R, w, dx, h)[0]
            assert u32(val[o]) != u32(without[o])                              # the ring-4 particle moved the value of voxel 0
    sim.close()


@pytest.fixture(scope="module")
def block():
    return block_and_scattered(24)


@pytest.mark.parametrize("R,w,dx,h", SETS)
def test_filled_block_and_scattered(fs, block, R, w, dx, h):
    """Leaf borders, the grid's edge, a -bg interior (third set), the SW == 0 branch inside the band (fourth); and never the spheres."""
    n = 24
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(block)
    sim.sdf_set_surface("averaged", h)
    g = snap(sim, R, w)
    val, act = check_avg(g, block, n, R, w, dx, h)
    assert (val[~act] < 0).any() == (R > w)
    sim.sdf_set_surface("spheres")
    s = snap(sim, R, w)
    sval, _ = check_grid(s, block, n, R, w, dx)
    if h >= R:
        assert (u32(val) != u32(sval)).any()
    assert set(map(tuple, g.origin.tolist())) <= set(map(tuple, s.origin.tolist()))     # its leaves are a subset of the spheres'
    # the same particles uploaded in another order: identical bytes
    sim.sdf_set_surface("averaged", h)
    sim.upload_particles(block[np.random.default_rng(3).permutation(len(block))])
    same_grid(snap(sim, R, w), g, "another order")
    sim.close()


def test_three_thousand_particles_in_one_cell(fs):
    """The sums far beyond 32 bits, and a z run longer than one chunk of the walk."""
    n, (R, w, dx, h) = 16, SETS[1]
    rng = np.random.default_rng(5)
    pos = np.vstack([np.array([1.0, -2.0, 3.0]) + rng.uniform(-0.5, 0.5, (3000, 3)), rng.uniform(-7.0, 7.0, (100, 3))])
    SW = sdf_avg_ref.sums(pos, n, h)[1]
    assert SW.max() > 2 ** 34
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    sim.sdf_set_surface("averaged", h)
    check_avg(snap(sim, R, w), pos, n, R, w, dx, h)
    sim.close()


def test_drop_scene_after_upload_and_steps(fs):
    n, (R, w, dx, h) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=0)
    sim = fs.FluidSim(n=n)
    sim.sdf_set_surface("averaged", h)
    sim.upload_particles(pos)
    check_avg(snap(sim, R, w), pos, n, R, w, dx, h, "after upload")
    for k in range(3):
        sim.step()
        g = snap(sim, R, w)
        p, _ = sim.download_particles()
        check_avg(g, p, n, R, w, dx, h, f"step {k}")
        assert 0 < g.n_leaves < sim.sdf_stats()["leaves_in_grid"]
    sim.close()


def test_what_follows_the_search_works_on_the_averaged_list(fs, block):
    """Mesh, filter and image of an averaged snapshot are the host functions' of the averaged list."""
    n, (R, w, dx, h) = 24, SETS[0]
    sim = fs.FluidSim(n=n)
    sim.upload_particles(block)
    spheres = snap(sim, R, w)
    sim.sdf_set_surface("averaged", h)
    g = snap(sim, R, w)
    check_avg(g, block, n, R, w, dx, h)
    sim.mesh_snapshot(R, w)
    hm = fs.sdf_mesh(g)
    assert len(hm.vertices) > 0
    same_mesh(sim.mesh_wait(), hm.vertices, hm.quads, "mesh")
    sm = fs.sdf_mesh(spheres)
    assert hm.vertices.shape != sm.vertices.shape or not np.array_equal(u32(hm.vertices), u32(sm.vertices))
    sim.sdf_snapshot(R, w, smooth=(1, 1))
    same_grid(sim.sdf_wait(), fs.sdf_filter(g, 1, 1), "filter")
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=32, height=32)
    sim.render_snapshot(R, w, cam, depth=True, normals=True)
    img = sim.render_wait()
    himg = fs.sdf_render(g, cam, None, True, True, True)
    assert img["n_hit"] == himg["n_hit"] > 0
    assert np.array_equal(img["rgb"], himg["rgb"]) and np.array_equal(u32(img["depth"]), u32(himg["depth"]))
    assert np.array_equal(u32(img["normals"]), u32(himg["normals"]))
    sim.close()


def test_back_to_the_spheres_and_the_refusals(fs, block):
    n, (R, w, dx, h) = 24, SETS[0]
    sim = fs.FluidSim(n=n)
    hd = sim._h
    sim.upload_particles(block)
    prm, g = fs.SdfParams(R, w), fs.SdfGridC()
    avg = fs.SdfSurface(1, 0, h)
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=16, height=8)
    # argument errors leave the setting as it was
    assert fs.lib.fluid_sdf_set_surface(None, C.byref(avg)) == ERR_ARG
    for kind, res, infl in ((2, 0, 3.0), (-1, 0, 3.0), (1, 1, 3.0), (1, 0, 0.0), (1, 0, -1.0), (1, 0, 4.5), (1, 0, float("nan"))):
        assert fs.lib.fluid_sdf_set_surface(hd, C.byref(fs.SdfSurface(kind, res, infl))) == ERR_ARG, (kind, res, infl)
        assert "influence" in fs.lib.fluid_last_error().decode()
    check_grid(snap(sim, R, w), block, n, R, w, dx)
    # under AVERAGED: attributes and rank records are refused, and leave no snapshot behind
    assert fs.lib.fluid_sdf_set_surface(hd, C.byref(avg)) == 0
    averaged = snap(sim, R, w)
    assert fs.lib.fluid_sdf_snapshot_attr(hd, C.byref(prm), None) == ERR_STATE
    assert "no attributes" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_mesh_snapshot_attr(hd, C.byref(prm), None) == ERR_STATE
    assert fs.lib.fluid_mesh_snapshot_ex(hd, C.byref(prm), None, int(fs.MESH.VELOCITY | fs.MESH.NORMALS)) == ERR_STATE
    assert fs.lib.fluid_dist_sdf_snapshot(hd, C.byref(prm)) == ERR_STATE
    assert "rank record" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_dist_sdf_snapshot_attr(hd, C.byref(prm)) == ERR_STATE
    assert fs.lib.fluid_sdf_wait(hd, C.byref(g)) == ERR_STATE
    m = fs.MeshC()
    assert fs.lib.fluid_mesh_wait(hd, C.byref(m)) == ERR_STATE
    assert fs.lib.fluid_mesh_snapshot_ex(hd, C.byref(prm), None, int(fs.MESH.NORMALS)) == 0          # without velocities it runs
    assert fs.lib.fluid_mesh_wait(hd, C.byref(m)) == 0 and m.n_vertices == len(fs.sdf_mesh(averaged).vertices)
    assert fs.lib.fluid_sdf_set_surface(hd, C.byref(fs.SdfSurface(7, 0, 3.0))) == ERR_ARG               # refused: still averaged
    same_grid(snap(sim, R, w), averaged, "after a refused setting")
    # back: kind 0 (whatever else the struct holds), then NULL
    assert fs.lib.fluid_sdf_set_surface(hd, C.byref(fs.SdfSurface(0, 9, -3.0))) == 0
    spheres = snap(sim, R, w)
    check_grid(spheres, block, n, R, w, dx)
    sim.sdf_snapshot(R, w, attr=True)                                                                   # and attributes are back
    same_grid(sim.sdf_wait_attr()[0], spheres, "attributes after the way back")
    assert fs.lib.fluid_dist_sdf_snapshot(hd, C.byref(prm)) == 0 and fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == 0
    sim.sdf_set_surface("averaged", h)
    sim.sdf_set_surface(None)
    same_grid(snap(sim, R, w), spheres, "NULL")
    sim.close()


def test_decomposed_handle_refuses_the_setting(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    assert fs.lib.fluid_sdf_set_surface(sim._h, C.byref(fs.SdfSurface(1, 0, 3.0))) == ERR_STATE
    assert "single-GPU" in fs.lib.fluid_last_error().decode()
    sim.close()


def test_driver_writes_the_averaged_surface(fs, tmp_path):
    """./run.sh fluid with FLUID_OUT_SURFACE=R,W and FLUID_OUT_SURFACE_KIND=averaged,H: surface<i>.vdb holds the reference's averaged
    grid for the particles of step i (taken from a handle that runs the same scene here); stdout is what it is without the two."""
    import os
    import subprocess
    import vdb_reader
    from sdf_testlib import FLUID, FLUID_VARS
    n, ppc, steps, (R, w, dx, h) = 16, 2, 2, SETS[0]
    lo, hi, _, _ = sdf_ref.geometry(n)
    outs = {}
    for mode in ("plain", "averaged"):
        d = tmp_path / mode
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k != "FLUID_OUT_SURFACE_KIND"}
        env.update(FLUID_N=str(n), FLUID_PPC=str(ppc), FLUID_STEPS=str(steps), FLUID_OUT=str(d / "simulation"))
        if mode == "averaged":
            env.update(FLUID_OUT_SURFACE=f"{R},{w}", FLUID_OUT_SURFACE_KIND=f"averaged,{h}")
        r = subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=d, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["plain"] == outs["averaged"]
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        sim.step()
        val, act = sdf_avg_ref.averaged(sim.download_particles()[0], n, R, w, dx, h)
        _, grids = vdb_reader.read(tmp_path / "averaged" / f"simulation/surface{i}.vdb")
        rv, ra = grids[0].dense(lo, hi)
        assert np.array_equal(u32(rv), u32(val)) and np.array_equal(ra, act), i
        assert sorted(grids[0].leaves) == [tuple(o) for o in sdf_ref.leaf_list(val, act, bg)[0].tolist()]
    sim.close()
