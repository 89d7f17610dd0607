"""GPU (-m gpu): the liquid surface (fluid_sdf_snapshot / _wait / _stats, kernels_sdf.hip) against tests/sdf_ref.py closed():
leaf origins, values (as bit patterns) and active masks must be equal exactly."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import sdf_ref
import vdb_reader
from sdf_testlib import u32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [(1.5, 2.5, 1.0), (3.0, 1.0, 1.0), (1.0, 2.0, 0.5), (2.0, 2.0, 1.0)]      # (R, w, dx)
LEAF_BYTES = 2048 + 64 + 12                                                    # FLUID_SDF_LEAF_BYTES
ERR_ARG, ERR_STATE = 1, 3


def check_grid(g, pos, n, R, w, dx):
    """g is exactly the leaf list of the reference's grid for the particles `pos`.  Returns the reference (values, active)."""
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert g.n == n and (g.background, g.radius, g.half_width) == (bg, fR, fw)
    assert g.n_leaves == len(org), (g.n_leaves, len(org))
    assert np.array_equal(g.origin, org)
    assert np.array_equal(g.active, a)
    assert np.array_equal(u32(g.values), u32(v))
    return val, act


def snap(sim, R, w):
    sim.sdf_snapshot(R, w)
    return sim.sdf_wait()


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [16, 25])
def test_one_particle(fs, n, R, w, dx):
    lo, hi, _, nl = sdf_ref.geometry(n)
    sim = fs.FluidSim(n=n, dx=dx)
    cases = {"voxel centre": [1.0, -2.0, 3.0], "generic": [0.3, -1.7, 2.25], "round tie": [1.5, -2.5, 0.5],
             "wall cell at hi": [hi - 0.2, hi + 0.3, hi], "outside": [hi + 0.6, 0.0, 0.0]}
    for name, p in cases.items():
        pos = np.array([p])
        sim.upload_particles(pos)
        g = snap(sim, R, w)
        val, act = check_grid(g, pos, n, R, w, dx)
        st = sim.sdf_stats()
        assert st == {"leaves_in_grid": nl ** 3, "leaves_listed": g.n_leaves, "bytes_to_host": g.n_leaves * LEAF_BYTES + 4}, name
        assert (g.n_leaves == 0) == (name == "outside"), name
        if name != "outside":
            dv, da = fs.sdf_to_dense(g)
            assert np.array_equal(u32(dv), u32(val)) and np.array_equal(da, act), name
            assert act.any(), name
    sim.close()


def test_ring_stop(fs):
    """A nearer particle in ring 2 behind a farther one in ring 1; and the ring-2 particle on the round tie with the minimum
    after ring 1 just above 1.5^2 — for voxel (0, 0, 0), mirrored to every axis and sign."""
    n, (R, w, dx) = 16, SETS[0]
    lo = sdf_ref.geometry(n)[0]
    sim = fs.FluidSim(n=n)
    base = [np.array([[1.45, 1.45, 1.45], [1.6, 0.0, 0.0]]), np.array([[1.4, 0.6, 0.0], [1.5, 0.0, 0.0]])]
    assert sdf_ref.base_cell(base[0]).tolist() == [[1, 1, 1], [2, 0, 0]] and sdf_ref.base_cell(base[1]).tolist() == [[1, 1, 0], [2, 0, 0]]
    for k, b in enumerate(base):
        for perm in itertools.permutations(range(3)):
            for sign in itertools.product((1.0, -1.0), repeat=3):
                pos = b[:, perm] * np.array(sign)
                sim.upload_particles(pos)
                g = snap(sim, R, w)
                val, act = check_grid(g, pos, n, R, w, dx)
                m = sdf_ref.dist2(0, 0, 0, pos).min()                     # the farther ring holds the minimum
                assert m == sdf_ref.dist2(0, 0, 0, pos[1]) and act[-lo, -lo, -lo]
                assert val[-lo, -lo, -lo] == np.float32(dx) * (np.sqrt(m) - np.float32(R))
    sim.close()


def test_filled_block_and_scattered(fs):
    """The interior's early stop beside band voxels, and leaves whose neighbourhood crosses the grid's edge."""
    n = 24
    lo, hi, _, _ = sdf_ref.geometry(n)
    rng = np.random.default_rng(24)
    c = np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    block = (np.repeat(c, 8, axis=0) + rng.uniform(-0.5, 0.5, (8 * len(c), 3)))
    pos = np.vstack([block, rng.uniform(lo - 1.0, hi + 1.0, (200, 3))])
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    for R, w, dx in (SETS[0], SETS[1], SETS[3]):
        val, act = check_grid(snap(sim, R, w), pos, n, R, w, dx)
        assert (val[~act] < 0).any() == (R > w)                            # deep inside the block: -bg where m <= min2
    sim.close()


def test_drop_scene_after_upload_and_steps(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=0)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    check_grid(snap(sim, R, w), pos, n, R, w, dx)
    for _ in range(3):
        sim.step()
        g = snap(sim, R, w)
        p, _ = sim.download_particles()
        check_grid(g, p, n, R, w, dx)
        assert 0 < g.n_leaves < sim.sdf_stats()["leaves_in_grid"]
    sim.close()


def test_slots_and_refusals(fs):
    n, (R, w, dx) = 32, SETS[0]
    sim = fs.FluidSim(n=n)
    h = sim._h
    g = fs.SdfGridC()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE                 # nothing outstanding
    for bad in ((2.0, 2.5), (1.5, 0.5), (0.0, 2.0), (-1.0, 2.0), (float("nan"), 2.0), (1.0, float("nan"))):
        assert fs.lib.fluid_sdf_snapshot(h, C.byref(fs.SdfParams(*bad))) == ERR_ARG, bad
    assert fs.lib.fluid_sdf_snapshot(h, None) == ERR_ARG
    sim.sdf_snapshot(R, w)                                                   # no particles at all: an empty list
    e = sim.sdf_wait()
    assert e.n_leaves == 0 and sim.sdf_stats()["bytes_to_host"] == 4
    p1 = fs.water_cube_drop(n, 4, seed=0)
    sim.upload_particles(p1)
    sim.sdf_snapshot(R, w)
    sim.step()
    p2, _ = sim.download_particles()
    sim.sdf_snapshot(2.0, 2.0)
    assert fs.lib.fluid_sdf_snapshot(h, C.byref(fs.SdfParams(R, w))) == ERR_STATE      # a third
    assert "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    g1, g2 = fs.SdfGridC(), fs.SdfGridC()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g1)) == 0 and fs.lib.fluid_sdf_wait(h, C.byref(g2)) == 0
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE

    def view(gc):
        k = gc.n_leaves
        org = np.ctypeslib.as_array(C.cast(gc.origin, C.POINTER(C.c_int32)), shape=(k, 3))
        val = np.ctypeslib.as_array(C.cast(gc.values, C.POINTER(C.c_float)), shape=(k, 512))
        wrd = np.ctypeslib.as_array(C.cast(gc.active, C.POINTER(C.c_uint64)), shape=(k, 8))
        act = np.unpackbits(wrd.view(np.uint8), axis=1, bitorder="little").astype(bool)
        return fs.SdfGrid(gc.n, org, val, act, gc.background, gc.radius, gc.half_width)
    # the first one's pointers are intact after the second snapshot and both waits
    check_grid(view(g1), p1, n, R, w, dx)
    check_grid(view(g2), p2, n, 2.0, 2.0, 1.0)
    st = sim.sdf_stats()
    assert st["leaves_listed"] == g2.n_leaves and st["bytes_to_host"] == g2.n_leaves * LEAF_BYTES + 4
    for _ in range(3):                                                        # the slots are reused
        sim.step()
        g = snap(sim, R, w)
        check_grid(g, sim.download_particles()[0], n, R, w, dx)
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    h = sim._h
    g, x = fs.SdfGridC(), C.c_int64()
    assert fs.lib.fluid_sdf_snapshot(h, C.byref(fs.SdfParams(1.5, 2.5))) == ERR_STATE
    assert "single-GPU" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_wait(h, C.byref(g)) == ERR_STATE
    assert fs.lib.fluid_sdf_stats(h, C.byref(x), None, None) == ERR_STATE
    sim.close()


def test_snapshots_do_not_disturb_the_steps(fs):
    """The same input on two handles: B takes a level-set snapshot after every step (and a density snapshot once); particles
    bit for bit and every field of the step stats — paths and cg_iters included — must come out as on A."""
    n, (R, w, _) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=3)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    a.upload_particles(pos)
    b.upload_particles(pos)
    sa, sb = [], []
    for k in range(4):
        sa.append(a.step())
        sb.append(b.step())
        b.sdf_snapshot(R, w)
        if k == 1:
            b.output_snapshot()
            assert b.output_wait().n_leaves > 0
        assert b.sdf_wait().n_leaves > 0
    assert sa == sb
    (pa, va), (pb, vb) = a.download_particles(), b.download_particles()
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    a.close(); b.close()


def test_driver_writes_the_surface(fs, tmp_path):
    """./run.sh fluid with FLUID_OUT_SURFACE=R,W: surface<i>.vdb holds the reference's grid for the particles of step i (taken
    from a handle that runs the same scene here), and the density files are what they are without the variable."""
    import leaf_ref
    n, ppc, steps, (R, w, dx) = 24, 4, 3, SETS[0]
    lo, hi, _, _ = sdf_ref.geometry(n)
    outs = {}
    for mode in ("plain", "surface"):
        d = tmp_path / mode
        d.mkdir()
        env = dict(os.environ, FLUID_N=str(n), FLUID_PPC=str(ppc), FLUID_STEPS=str(steps), FLUID_OUT=str(d / "simulation"))
        for k in ("FLUID_OUT_SURFACE", "FLUID_OUT_DENSE", "FLUID_BLOCKS", "FLUID_SOURCE_EVERY", "FLUID_RAW"):
            env.pop(k, None)
        if mode == "surface":
            env["FLUID_OUT_SURFACE"] = f"{R},{w}"
        r = subprocess.run([os.path.join(ROOT, "run.sh"), "fluid"], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["plain"] == outs["surface"]
    for nm in ["mygrids.vdb"] + [f"simulation/mygrids{i}.vdb" for i in range(steps)]:
        assert leaf_ref.same_file(tmp_path / "plain" / nm, tmp_path / "surface" / nm), nm
    assert not list((tmp_path / "plain" / "simulation").glob("surface*"))
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    bg = sdf_ref.constants(R, w, dx)[3]
    for i in range(steps):
        sim.step()
        val, act = sdf_ref.closed(sim.download_particles()[0], n, R, w, dx)
        _, grids = vdb_reader.read(tmp_path / "surface" / f"simulation/surface{i}.vdb")
        assert len(grids) == 1 and grids[0].name == "surface" and grids[0].metadata["class"] == "level set"
        assert np.float32(grids[0].background) == bg
        rv, ra = grids[0].dense(lo, hi)
        assert np.array_equal(u32(rv), u32(val)) and np.array_equal(ra, act), i
        assert sorted(grids[0].leaves) == [tuple(o) for o in sdf_ref.leaf_list(val, act, bg)[0].tolist()]
    sim.close()
