"""GPU (-m gpu): the velocity trails (fluid_sdf_set_trails, kernels_sdf_trail.hip) against tests/sdf_trail_ref.py: leaf origins,
masks and values (as bit patterns) must be equal exactly; the ways back to the spheres; a device-to-device cross-check at constant
radius; what follows the search (filter, mesh, image) against the host functions on the trails' list; the refusals."""
import ctypes as C

import numpy as np
import pytest

import sdf_ref
import sdf_trail_ref as ref
from sdf_testlib import same_grid, same_mesh, u32
from test_gpu_sdf import check_grid

pytestmark = pytest.mark.gpu

SETS = ref.SETS
ERR_ARG, ERR_STATE = 1, 3
F = np.float32


def check_dense(g, val, act, n, R, w, dx, what=""):
    """g is exactly the leaf list of the dense reference (val, act)."""
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert g.n == n and (g.background, g.radius, g.half_width) == (bg, fR, fw), what
    assert g.n_leaves == len(org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.origin, org), what
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), what


def check_trails(g, pos, vel, n, R, w, dx, trails, what=""):
    """g is exactly the leaf list of the reference's grid for the trails of (pos, vel).  Returns (values, active, instances)."""
    P, r, _ = ref.instances(pos, vel, R, trails)
    val, act = ref.union(P, r, n, R, w, dx)
    check_dense(g, val, act, n, R, w, dx, what)
    return val, act, len(P)


def snap(sim, R, w):
    sim.sdf_snapshot(R, w)
    return sim.sdf_wait()


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [16, 25])
def test_one_moving_particle(fs, n, R, w, dx):
    lo, hi, _, _ = sdf_ref.geometry(n)
    t = ref.trails_of(R)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.sdf_set_trails(*t)
    corner = [0.3, -0.2, 0.4]                                           # (0, 0, 0) is a corner of eight leaves
    s = 5.0
    cases = {f"{'+-'[k & 1]}{'xyz'[k >> 1]}": (corner, np.eye(3)[k >> 1] * (s if k & 1 == 0 else -s)) for k in range(6)}
    cases["diagonal"] = (corner, [3.0, -3.0, 3.0])
    cases["through the leaf corner"] = ([2.1, 1.9, 2.2], [3.0, 3.0, 3.0])
    cases["slow: one instance"] = (corner, [0.1, 0.0, 0.0])
    cases["head in the wall cell at hi, tail leaving"] = ([hi - 0.2, hi + 0.3, hi], [-4.0, -4.0, 0.0])
    cases["outside, tail coming in"] = ([hi + 2.0, 0.2, -0.3], [6.0, 0.0, 0.0])
    cases["outside, tail staying out"] = ([hi + 2.0, 0.2, -0.3], [-6.0, 0.0, 0.0])
    for name, (p, v) in cases.items():
        pos, vel = np.array([p]), np.array([v], dtype=np.float64)
        sim.upload_particles(pos, vel)
        g = snap(sim, R, w)
        _, act, k = check_trails(g, pos, vel, n, R, w, dx, t, name)
        assert sim.sdf_trails_stats() == {"particles": 1, "instances": k}, name
        assert (k == 1) == name.startswith("slow"), (name, k)
        assert (g.n_leaves == 0) == name.endswith("staying out"), name
        if name.endswith("coming in"):
            assert act.any() and not sdf_ref.closed(pos, n, R, w, dx)[1].any()      # the particle itself does not count
    sim.close()


def test_the_way_back(fs):
    """Zero velocities, max_instances = 1 and the setting cleared: the bytes of the spheres' snapshot on the same handle."""
    n, (R, w, dx) = 24, SETS[1]
    pos, vel = ref.block_scene(n)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    spheres = snap(sim, R, w)
    check_grid(spheres, pos, n, R, w, dx)
    sim.sdf_set_trails(1.0, 1.0, R / 2, 1)
    same_grid(snap(sim, R, w), spheres, "max_instances = 1")
    assert sim.sdf_trails_stats() == {"particles": len(pos), "instances": len(pos)}
    sim.sdf_set_trails(0.0, 1.0, R / 2, 8)
    same_grid(snap(sim, R, w), spheres, "shutter 0")
    sim.sdf_set_trails(*ref.trails_of(R))
    moved = snap(sim, R, w)
    assert moved.n_leaves >= spheres.n_leaves and not (moved.values.shape == spheres.values.shape and np.array_equal(u32(moved.values), u32(spheres.values)))
    sim.upload_particles(pos, np.zeros_like(pos))
    same_grid(snap(sim, R, w), spheres, "zero velocities")
    sim.upload_particles(pos, vel)
    sim.sdf_set_trails(None)
    same_grid(snap(sim, R, w), spheres, "cleared")
    sim.sdf_snapshot(R, w, attr=True)                                   # and attributes are back
    same_grid(sim.sdf_wait_attr()[0], spheres, "attributes after the way back")
    sim.close()


@pytest.mark.parametrize("R,w,dx", SETS)
def test_constant_radius_is_the_spheres_of_the_instances(fs, R, w, dx):
    """Rm = R: the bytes of a spheres' snapshot of a second handle whose particles are the host-expanded instances (no numpy in it)."""
    n = 24
    pos, vel = ref.block_scene(n)
    t = (1.0, 1.0, R, 8)
    a, b = fs.FluidSim(n=n, dx=dx), fs.FluidSim(n=n, dx=dx)
    a.upload_particles(pos, vel)
    a.sdf_set_trails(*t)
    P, r = fs.particles_trails(pos, vel, R, w, *t)
    assert len(P) > 2 * len(pos) and (r == F(R)).all()
    b.upload_particles(P)
    ga, gb = snap(a, R, w), snap(b, R, w)
    assert ga.n_leaves > 0
    same_grid(ga, gb)
    assert a.sdf_trails_stats()["instances"] == len(P)
    a.close(), b.close()


@pytest.mark.parametrize("R,w,dx", SETS)
def test_filled_block_and_scattered(fs, R, w, dx):
    """Leaf borders, the grid's edge, tails that leave and enter the grid, a -bg interior (third set); any order; the stats."""
    n = 24
    pos, vel = ref.block_scene(n)
    val, act, k = ref.block_reference(R, w, dx, n)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    sim.sdf_set_trails(*ref.trails_of(R))
    g = snap(sim, R, w)
    check_dense(g, val, act, n, R, w, dx)
    assert (val[~act] < 0).any() == (R > w)
    host = fs.lib.fluid_particles_trails(len(pos), pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p), C.byref(fs.SdfParams(R, w)),
                                         C.byref(fs.SdfTrails(*ref.trails_of(R), 0)), 0, None, None)
    assert sim.sdf_trails_stats() == {"particles": len(pos), "instances": host} and host == k
    o = np.random.default_rng(3).permutation(len(pos))
    sim.upload_particles(pos[o], vel[o])
    same_grid(snap(sim, R, w), g, "another order")
    sim.close()


def test_three_thousand_slow_particles_in_one_cell(fs):
    """Runs longer than one 64-item chunk of the walk and many instances per cell, beside 100 scattered fast particles."""
    n, (R, w, dx) = 16, SETS[1]
    rng = np.random.default_rng(5)
    pos = np.vstack([np.array([1.0, -2.0, 3.0]) + rng.uniform(-0.5, 0.5, (3000, 3)), rng.uniform(-7.0, 7.0, (100, 3))])
    vel = np.vstack([rng.normal(size=(3000, 3)) * 0.6, rng.normal(size=(100, 3)) * 4.0])
    t = ref.trails_of(R)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    sim.sdf_set_trails(*t)
    _, _, k = check_trails(snap(sim, R, w), pos, vel, n, R, w, dx, t)
    assert k > len(pos) + 1000                                          # the slow ones leave a second instance in their own cell
    sim.close()


def test_after_real_steps(fs):
    """A 6^3 cube of particles, thrown sideways at 3.6 voxels per time, falls for three steps; shutter = the step's dt, on the
    downloaded positions and velocities.  (Free fall alone reaches 1 voxel per time by then: 0.1 voxel of path, below the first
    step c * R = 0.125 of a trail, which would leave every particle one instance.)"""
    n, (R, w, dx) = 24, SETS[0]
    rng = np.random.default_rng(6)
    c = np.stack(np.meshgrid(*[np.arange(-3, 3)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = c + np.array([0.0, 3.0, 0.0]) + rng.uniform(-0.4, 0.4, c.shape)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, np.tile([3.0, 0.0, 2.0], (len(pos), 1)))
    for _ in range(3):
        st = sim.step()
    p, v = sim.download_particles()
    t = (st["dt_out"], 0.25, R / 2, 16)
    sim.sdf_set_trails(*t)
    _, _, k = check_trails(snap(sim, R, w), p, v, n, R, w, dx, t)
    print(f"dt {st['dt_out']}, fastest {np.linalg.norm(v, axis=1).max()} voxels per time, {k} instances of {len(p)} particles")
    assert len(p) == len(pos) and k > len(p)                            # about 0.36 voxel of path against a first step of 0.125
    sim.close()


def test_what_follows_the_search_works_on_the_trails_list(fs):
    """Mesh with normals and triangles, image, box filter and the grown HJWENO5 track are the host functions' of the trails' list."""
    n, (R, w, dx) = 24, SETS[0]
    pos, vel = ref.block_scene(n)
    val, act, _ = ref.block_reference(R, w, dx, n)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    spheres = snap(sim, R, w)
    sim.sdf_set_trails(*ref.trails_of(R))
    g = snap(sim, R, w)
    check_dense(g, val, act, n, R, w, dx)
    sim.mesh_snapshot(R, w, normals=True, triangles=True)
    mv, mq, parts = sim.mesh_wait_ex()
    hm = fs.sdf_mesh(g)
    assert len(hm.vertices) > 0
    same_mesh((mv, mq), hm.vertices, hm.quads, "mesh")
    assert np.array_equal(u32(parts["normals"]), u32(fs.sdf_mesh_normals(g))) and np.array_equal(parts["triangles"], fs.mesh_triangles(mv, mq))
    sm = fs.sdf_mesh(spheres)
    assert hm.vertices.shape != sm.vertices.shape or not np.array_equal(u32(hm.vertices), u32(sm.vertices))
    sim.mesh_snapshot(R, w)
    same_mesh(sim.mesh_wait(), hm.vertices, hm.quads, "plain mesh")
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=32, height=32)
    sim.render_snapshot(R, w, cam, depth=True, normals=True)
    img = sim.render_wait()
    himg = fs.sdf_render(g, cam, None, True, True, True)
    assert img["n_hit"] == himg["n_hit"] > 0
    assert np.array_equal(img["rgb"], himg["rgb"]) and np.array_equal(u32(img["depth"]), u32(himg["depth"]))
    assert np.array_equal(u32(img["normals"]), u32(himg["normals"]))
    sim.sdf_snapshot(R, w, smooth=(1, 1))
    same_grid(sim.sdf_wait(), fs.sdf_filter(g, 1, 1), "box filter")
    sim.mesh_snapshot(R, w, smooth=(1, 1))
    fm = fs.sdf_mesh(fs.sdf_filter(g, 1, 1))
    same_mesh(sim.mesh_wait(), fm.vertices, fm.quads, "filtered mesh")
    filt = (1, 2, 0.5 * dx)
    sim.sdf_set_track(3, True, grow=True, scheme="hjweno5")
    sim.sdf_snapshot(R, w, smooth=filt)
    same_grid(sim.sdf_wait(), fs.sdf_filter_grown(g, filt, (3, True, "hjweno5")), "grown HJWENO5 track")
    sim.close()


def avg_record(sim, R, w, h):
    sim.sdf_snapshot_avg(R, w, h)
    p = sim.sdf_wait_avg()
    return p.origin.tobytes() + p.dist2.tobytes() + p.sums.tobytes()


def test_refusals_and_state_rules(fs):
    n, (R, w, dx) = 24, SETS[0]
    pos, vel = ref.block_scene(n)
    sim, other = fs.FluidSim(n=n), fs.FluidSim(n=n)
    hd = sim._h
    sim.upload_particles(pos, vel), other.upload_particles(pos, vel)
    prm, g, m = fs.SdfParams(R, w), fs.SdfGridC(), fs.MeshC()
    good = fs.SdfTrails(1.0, 1.0, R / 2, 8, 0)
    cam = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=16, height=8)
    spheres, other_before = snap(sim, R, w), snap(other, R, w)
    record = avg_record(sim, R, w, 3.0)
    # argument errors leave the setting as it was: off
    assert fs.lib.fluid_sdf_set_trails(None, C.byref(good)) == ERR_ARG
    nan, inf = float("nan"), float("inf")
    for bad in ((-1.0, 1.0, 0.5, 8, 0), (nan, 1.0, 0.5, 8, 0), (inf, 1.0, 0.5, 8, 0), (1.0, 0.0, 0.5, 8, 0), (1.0, nan, 0.5, 8, 0), (1.0, inf, 0.5, 8, 0),
                (1.0, 1.0, 0.0, 8, 0), (1.0, 1.0, nan, 8, 0), (1.0, 1.0, 0.5, 0, 0), (1.0, 1.0, 0.5, 33, 0), (1.0, 1.0, 0.5, 8, 1)):
        assert fs.lib.fluid_sdf_set_trails(hd, C.byref(fs.SdfTrails(*bad))) == ERR_ARG, bad
        assert "max_instances" in fs.lib.fluid_last_error().decode()
    same_grid(snap(sim, R, w), spheres, "after refused settings")
    # Rm <= R belongs to the snapshot: every entry point refuses, and leaves no snapshot behind
    assert fs.lib.fluid_sdf_set_trails(hd, C.byref(fs.SdfTrails(1.0, 1.0, 1.5, 8, 0))) == 0
    assert fs.lib.fluid_sdf_snapshot(hd, C.byref(prm)) == ERR_ARG and "radius_min" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_snapshot_filtered(hd, C.byref(prm), C.byref(fs.SdfFilter(1, 1, 0.0))) == ERR_ARG
    assert fs.lib.fluid_mesh_snapshot(hd, C.byref(prm)) == ERR_ARG
    assert fs.lib.fluid_render_snapshot(hd, C.byref(prm), None, C.byref(cam), None, int(fs.RENDER.RGB)) == ERR_ARG
    assert fs.lib.fluid_sdf_wait(hd, C.byref(g)) == ERR_STATE and fs.lib.fluid_mesh_wait(hd, C.byref(m)) == ERR_STATE
    assert fs.lib.fluid_sdf_snapshot(hd, C.byref(fs.SdfParams(1.5, 2.5))) == 0 and fs.lib.fluid_sdf_wait(hd, C.byref(g)) == 0      # R = 1.5 admits it
    # under trails: attributes and the spheres' rank records are refused, and leave no snapshot behind
    assert fs.lib.fluid_sdf_set_trails(hd, C.byref(good)) == 0
    trails = snap(sim, R, w)
    assert trails.n_leaves >= spheres.n_leaves
    assert fs.lib.fluid_sdf_snapshot_attr(hd, C.byref(prm), None) == ERR_STATE
    assert "no attributes" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_mesh_snapshot_attr(hd, C.byref(prm), None) == ERR_STATE
    assert fs.lib.fluid_mesh_snapshot_ex(hd, C.byref(prm), None, int(fs.MESH.VELOCITY | fs.MESH.NORMALS)) == ERR_STATE
    assert fs.lib.fluid_dist_sdf_snapshot(hd, C.byref(prm)) == ERR_STATE
    assert "rank record" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_dist_sdf_snapshot_attr(hd, C.byref(prm)) == ERR_STATE
    assert fs.lib.fluid_sdf_wait(hd, C.byref(g)) == ERR_STATE and fs.lib.fluid_mesh_wait(hd, C.byref(m)) == ERR_STATE
    assert fs.lib.fluid_mesh_snapshot_ex(hd, C.byref(prm), None, int(fs.MESH.NORMALS)) == 0          # without velocities it runs
    assert fs.lib.fluid_mesh_wait(hd, C.byref(m)) == 0 and m.n_vertices == len(fs.sdf_mesh(trails).vertices)
    # the averaged rank record takes its surface as an argument: the same bytes, and the setting stays
    assert avg_record(sim, R, w, 3.0) == record
    same_grid(snap(sim, R, w), trails, "after an averaged rank record")
    # trails and the averaged surface exclude each other, whichever comes second
    assert fs.lib.fluid_sdf_set_surface(hd, C.byref(fs.SdfSurface(1, 0, 3.0))) == ERR_STATE
    assert "exclude" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_set_surface(hd, C.byref(fs.SdfSurface(0, 0, 0.0))) == 0
    same_grid(snap(sim, R, w), trails, "after a refused surface")
    assert fs.lib.fluid_sdf_set_trails(hd, None) == 0
    assert fs.lib.fluid_sdf_set_surface(hd, C.byref(fs.SdfSurface(1, 0, 3.0))) == 0
    averaged = snap(sim, R, w)
    assert fs.lib.fluid_sdf_set_trails(hd, C.byref(good)) == ERR_STATE and "exclude" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_set_trails(hd, None) == 0                                                 # clearing is always allowed
    same_grid(snap(sim, R, w), averaged, "after a refused setting")
    sim.sdf_set_surface(None)
    same_grid(snap(sim, R, w), spheres, "everything cleared")
    assert fs.lib.fluid_dist_sdf_snapshot(hd, C.byref(prm)) == 0 and fs.lib.fluid_dist_sdf_wait(hd, C.byref(g)) == 0
    assert sim.sdf_trails_stats()["particles"] == len(pos)                                            # of the last snapshot under the setting
    # the other handle never noticed
    assert other.sdf_trails_stats() == {"particles": 0, "instances": 0}
    same_grid(snap(other, R, w), other_before, "a second handle")
    with pytest.raises(fs.FluidError):
        sim.sdf_set_trails(1.0, max_instances=40)
    sim.close(), other.close()


def test_decomposed_handle_refuses_the_setting(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    assert fs.lib.fluid_sdf_set_trails(sim._h, C.byref(fs.SdfTrails(1.0, 1.0, 0.5, 8, 0))) == ERR_STATE
    assert "single-GPU" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_set_trails(sim._h, None) == ERR_STATE
    assert fs.lib.fluid_sdf_trails_stats(sim._h, None, None) == ERR_STATE
    sim.close()


def test_driver_writes_the_trails(fs, tmp_path):
    """./run.sh fluid with FLUID_OUT_SURFACE=R,W and FLUID_OUT_SURFACE_TRAILS=dt: surface<i>.vdb holds the reference's grid for the
    particles and velocities of step i and its dt (taken from a handle that runs the same scene here); stdout is what it is without."""
    import os
    import subprocess
    import vdb_reader
    from sdf_testlib import FLUID, FLUID_VARS
    n, ppc, steps, (R, w, dx) = 16, 2, 2, (1.5, 2.0, 1.0)
    lo, hi, _, _ = sdf_ref.geometry(n)
    outs = {}
    for mode in ("plain", "trails"):
        d = tmp_path / mode
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k not in ("FLUID_OUT_SURFACE_KIND", "FLUID_OUT_SURFACE_TRAILS")}
        env.update(FLUID_N=str(n), FLUID_PPC=str(ppc), FLUID_STEPS=str(steps), FLUID_OUT=str(d / "simulation"))
        if mode == "trails":
            env.update(FLUID_OUT_SURFACE=f"{R},{w}", FLUID_OUT_SURFACE_TRAILS="dt,0.5")
        r = subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=d, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["plain"] == outs["trails"]
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        st = sim.step()
        p, v = sim.download_particles()
        val, act = ref.trails_surface(p, v, n, R, w, dx, (st["dt_out"], 0.5, R / 2, 16))
        _, grids = vdb_reader.read(tmp_path / "trails" / f"simulation/surface{i}.vdb")
        rv, ra = grids[0].dense(lo, hi)
        assert np.array_equal(u32(rv), u32(val)) and np.array_equal(ra, act), i
        assert sorted(grids[0].leaves) == [tuple(o) for o in sdf_ref.leaf_list(val, act, bg)[0].tolist()]
    sim.close()
