"""GPU (-m gpu): leaf snapshots of the output grid (fluid_output_snapshot / _wait / _stats, kernels_output.hip) against the
dense field downloaded from the same handle, compared as bit patterns; the leaf lists they are checked against are made
in numpy (tests/leaf_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import leaf_ref
from sdf_testlib import u32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF_BYTES, HEADER_BYTES = 2048 + 12, 4      # FLUID_OUTPUT_LEAF_BYTES, FLUID_OUTPUT_HEADER_BYTES


def check_snapshot(fs, sim, lg, dense, strictly_sparse=True):
    """lg is exactly the leaf list of `dense` (the field downloaded when the snapshot was taken)."""
    n = dense.shape[0]
    _, _, _, nl = leaf_ref.geometry(n)
    org, val = leaf_ref.leaf_list(dense)
    assert lg.n == n and lg.n_leaves == len(org)
    assert np.array_equal(lg.origin, org)          # the listed leaves are those with a non-zero bit pattern, and no others
    assert np.array_equal(u32(lg.values), u32(val))            # ... with +0 outside the grid
    o = lg.origin.astype(np.int64)
    key = (o[:, 0] * 4096 + o[:, 1]) * 4096 + o[:, 2]
    assert (np.diff(key) > 0).all()                # strictly ascending (x, y, z)
    assert np.array_equal(u32(fs.leaves_to_dense(lg)), u32(dense))
    if strictly_sparse:
        assert 0 < lg.n_leaves < nl ** 3
    st = sim.output_stats()
    assert st["leaves_in_grid"] == nl ** 3 and st["leaves_listed"] == lg.n_leaves
    assert st["bytes_to_host"] == lg.n_leaves * LEAF_BYTES + HEADER_BYTES


def snapshot(sim):
    sim.output_snapshot()
    return sim.output_wait()


@pytest.mark.parametrize("n", [32, 64, 72, 121])   # 72: off = -4 and 10 leaves per axis, the mark kernel's z loop makes a second, partial trip
def test_drop_scene(fs, n):
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 4, seed=0))
    for k in range(3):
        sim.step()
        if k in (0, 2):
            check_snapshot(fs, sim, snapshot(sim), sim.field(fs.FIELD.OUTPUT))
    sim.close()


def test_snapshot_overlaps_the_next_step(fs):
    n = 64
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 8, seed=1))
    for _ in range(2):
        sim.step()
    before = sim.field(fs.FIELD.OUTPUT)
    sim.output_snapshot()
    sim.step()                                     # before the wait: clears and refills the grid
    after = sim.field(fs.FIELD.OUTPUT)
    assert not np.array_equal(u32(before), u32(after))
    lg = sim.output_wait()
    assert np.array_equal(u32(fs.leaves_to_dense(lg)), u32(before))
    assert np.array_equal(lg.origin, leaf_ref.leaf_list(before)[0])
    sim.close()


def test_two_in_flight_come_back_in_order(fs):
    n = 32
    sim = fs.FluidSim(n=n)
    h = sim._h
    g = fs.LeafGridC()
    assert fs.lib.fluid_output_wait(h, C.byref(g)) == 3            # nothing outstanding: FLUID_ERR_STATE
    sim.upload_particles(fs.water_cube_drop(n, 4, seed=0))
    sim.step()
    d1 = sim.field(fs.FIELD.OUTPUT)
    sim.output_snapshot()
    sim.step()
    d2 = sim.field(fs.FIELD.OUTPUT)
    sim.output_snapshot()
    assert not np.array_equal(u32(d1), u32(d2))
    assert fs.lib.fluid_output_snapshot(h) == 3                    # a third: FLUID_ERR_STATE
    assert "two output snapshots" in fs.lib.fluid_last_error().decode()
    l1, l2 = sim.output_wait(), sim.output_wait()
    assert np.array_equal(u32(fs.leaves_to_dense(l1)), u32(d1)) and np.array_equal(u32(fs.leaves_to_dense(l2)), u32(d2))
    assert fs.lib.fluid_output_wait(h, C.byref(g)) == 3
    # the slots are reused: many more rounds on the same handle
    for _ in range(3):
        sim.step()
        check_snapshot(fs, sim, snapshot(sim), sim.field(fs.FIELD.OUTPUT))
    sim.close()


def uploaded_fields(n):
    """Containers with non-zeros far outside any particle's box."""
    rng = np.random.default_rng(n)
    _, _, _, nl = leaf_ref.geometry(n)
    zero = np.zeros((n, n, n), np.float32)
    c0 = zero.copy(); c0[0, 0, 0] = 3.25
    c1 = zero.copy(); c1[n - 1, n - 1, n - 1] = -7.5
    nz = zero.copy(); nz[n // 2, 1, n - 2] = -0.0
    r = np.where(rng.random((n, n, n)) < 0.002, rng.standard_normal((n, n, n)).astype(np.float32), np.float32(0))
    r = np.ascontiguousarray(r, dtype=np.float32)
    r[0, n - 1, 0] = np.nan
    r[n - 1, 0, n - 1] = 1e-45                                     # the smallest subnormal
    lo, _, l0, _ = leaf_ref.geometry(n)
    off = lo - l0
    r[max(0, 8 - off):16 - off, :, :] = 0                          # a slab of leaves stays unlisted
    return {"corner_first": c0, "corner_last": c1, "negative_zero": nz, "random_sparse": r, "zero": zero}


@pytest.mark.parametrize("n", [121, 64])
def test_uploaded_containers(fs, n):
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 2, seed=0))
    sim.step()
    for name, f in uploaded_fields(n).items():
        sim.upload_field(fs.FIELD.CONTAINER, f)
        lg = snapshot(sim)
        dense = sim.field(fs.FIELD.OUTPUT)
        assert np.array_equal(u32(dense), u32(f)), name
        check_snapshot(fs, sim, lg, f, strictly_sparse=name != "zero")
        if name == "zero":
            assert lg.n_leaves == 0 and sim.output_stats()["bytes_to_host"] == HEADER_BYTES
        elif name != "random_sparse":
            assert lg.n_leaves == 1, name
    sim.close()


def test_obstacle_scene_and_reused_handle(fs):
    n = 48
    solid = np.zeros((n, n, n), np.uint8)
    solid[:2] = solid[-2:] = 1
    solid[:, :2] = solid[:, -2:] = 1
    solid[:, :, :2] = solid[:, :, -2:] = 1
    solid[18:30, 6:12, 18:30] = 1                                  # a block under the falling cube
    sim = fs.FluidSim(n=n)
    sim.set_solid(solid)
    sim.upload_particles(fs.water_cube_drop(n, 4, seed=0))
    for _ in range(3):
        sim.step()
    check_snapshot(fs, sim, snapshot(sim), sim.field(fs.FIELD.OUTPUT))
    pos = fs.water_cube_drop(n, 4, seed=5) + np.array([6.0, 3.0, -5.0])
    sim.upload_particles(pos)                                      # the handle again, other particles
    for _ in range(2):
        sim.step()
        check_snapshot(fs, sim, snapshot(sim), sim.field(fs.FIELD.OUTPUT))
    sim.close()


def test_two_handles_give_the_same_bytes(fs):
    n = 64
    pos = fs.water_cube_drop(n, 8, seed=2)
    got = []
    for _ in range(2):
        sim = fs.FluidSim(n=n)
        sim.upload_particles(pos)
        for _ in range(3):
            sim.step()
        lg = snapshot(sim)
        got.append((lg.origin.tobytes(), lg.values.tobytes()))
        sim.close()
    assert got[0] == got[1]


def test_leaf_file_is_the_dense_file_after_a_step(fs, tmp_path):
    n = 121
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 4, seed=0))
    sim.step()
    lg = snapshot(sim)
    fs.write_vdb_leaves(tmp_path / "leaves.vdb", lg)
    fs.write_vdb(tmp_path / "dense.vdb", sim.field(fs.FIELD.OUTPUT))
    assert leaf_ref.same_file(tmp_path / "leaves.vdb", tmp_path / "dense.vdb")
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    h = sim._h
    g, x = fs.LeafGridC(), C.c_int64()
    assert fs.lib.fluid_output_snapshot(h) == 3
    assert "single-GPU" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_output_wait(h, C.byref(g)) == 3
    assert fs.lib.fluid_output_stats(h, C.byref(x), None, None) == 3
    sim.close()


def test_driver_writes_the_same_files_either_way(fs, tmp_path):
    """./run.sh fluid with the leaf snapshots and a writer thread (default) and with FLUID_OUT_DENSE=1 (download, two dense writes)."""
    steps = 3
    outs = {}
    for mode in ("leaves", "dense"):
        d = tmp_path / mode
        d.mkdir()
        env = dict(os.environ, FLUID_N="32", FLUID_PPC="4", FLUID_STEPS=str(steps), FLUID_RAW="1", FLUID_OUT=str(d / "simulation"))
        env.pop("FLUID_OUT_DENSE", None)
        if mode == "dense":
            env["FLUID_OUT_DENSE"] = "1"
        r = subprocess.run([os.path.join(ROOT, "run.sh"), "fluid"], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["leaves"] == outs["dense"] and sum(ln.startswith("Iteration:") for ln in outs["dense"]) == steps
    names = ["mygrids.vdb"] + [f"simulation/mygrids{i}.vdb" for i in range(steps)]
    for nm in names:
        assert leaf_ref.same_file(tmp_path / "leaves" / nm, tmp_path / "dense" / nm), nm
    for i in range(steps):
        a = open(tmp_path / "leaves" / f"simulation/mygrids{i}.f32", "rb").read()
        b = open(tmp_path / "dense" / f"simulation/mygrids{i}.f32", "rb").read()
        assert a == b and len(a) == 4 + 4 * 32 ** 3
        assert np.frombuffer(a, np.float32, offset=4).any()        # the scene is there
