"""GPU (-m gpu): leaf snapshots of the OWNED BLOCK of a decomposed handle (fluid_dist_output_snapshot / _wait / _stats / _every,
kernels_output.hip) and their merge (fluid_leaf_grids_merge).  Blocks run as threads of a LocalGroup on the one GPU of the box,
as in tests/test_gpu_dist.py.  The reference of every list is the same handle's own dense download at the moment of the
snapshot, turned into a leaf list in numpy (tests/leaf_ref.py) — never another snapshot."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import leaf_ref
import vdb_reader
from conftest import rel_l2, ROOT
from sdf_testlib import fluid_env, u32

pytestmark = pytest.mark.gpu

LEAF_BYTES, HEADER_BYTES = 2048 + 12, 4      # FLUID_OUTPUT_LEAF_BYTES, FLUID_OUTPUT_HEADER_BYTES
ERR_STATE = 3
REBALANCED = 32                              # FLUID_PATH_DIST_REBALANCED


def keys_of(origin):
    return set(map(tuple, np.asarray(origin).reshape(-1, 3).tolist()))


def ascending(origin):
    o = origin.astype(np.int64)
    key = (o[:, 0] * 8192 + o[:, 1]) * 8192 + o[:, 2]
    return (np.diff(key) > 0).all()


def leaves_meeting(n, own_lo, own_hi):
    """Global leaves that intersect the owned block [own_lo, own_hi) (array indices)."""
    lo, _, l0, _ = leaf_ref.geometry(n)
    off = l0 - lo
    k = 1
    for a in range(3):
        k *= (own_hi[a] - 1 - off) // 8 - (own_lo[a] - off) // 8 + 1
    return k


def own_slices(sim):
    return tuple(slice(sim.own_lo[k], sim.own_hi[k]) for k in range(3))


def check_rank_list(fs, sim, lg, block):
    """lg is exactly the leaf list of the global-size array that is zero but for this rank's owned block."""
    n = sim.n
    g = np.zeros((n, n, n), np.float32)
    g[own_slices(sim)] = block
    org, val = leaf_ref.leaf_list(g)
    assert lg.n == n and lg.n_leaves == len(org)
    assert np.array_equal(lg.origin, org)
    assert np.array_equal(u32(lg.values), u32(val))        # +0 in every voxel this rank does not own
    assert ascending(lg.origin)


def run_group(fs, dims, n, cuts, mode, work, pos, **kw):
    """work(sim, r) on every rank of a LocalGroup; returns (sims' geometry, results by rank)."""
    fd = fs.load_dist()
    size = dims[0] * dims[1] * dims[2]
    grp = fd.LocalGroup(size)
    sims = [None] * size

    def run(r):
        sim = fd.DistFluidSim(n, dims, cuts, grp.comms[r], dist_solve=mode, **kw)
        sims[r] = sim
        return work(sim, r)

    try:
        res = grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    return sims, res


CASES = [
    # n, dims, cuts (None: partition_blocks; an axis None: that axis from partition_blocks), scene offset
    (32, (2, 1, 1), [[0, 20, 32], [0, 32], [0, 32]]),                 # off = 0, leaf 16..23 split at 20
    (33, (2, 1, 2), [None, [0, 33], [0, 20, 33]]),                    # odd N, unaligned rows, last leaf with one in-grid cell
    (50, (2, 2, 1), None),                                            # off = -7: every cut at a multiple of 4 splits a leaf
    (48, (2, 2, 2), [[0, 20, 48]] * 3),                               # one leaf shared by eight ranks
    (121, (2, 1, 1), [[0, 64, 121], [0, 121], [0, 121]]),             # the reference's grid, off = -4
]


@pytest.mark.parametrize("mode", ["decomposed", "replicated"])
@pytest.mark.parametrize("n,dims,cuts", CASES, ids=[f"n{c[0]}" for c in CASES])
def test_block_lists_and_their_merge(fs, mode, n, dims, cuts):
    fd = fs.load_dist()
    F = fs.FIELD
    pos = fs.water_cube_drop(n, 4, seed=0)
    auto = fd.partition_blocks(n, pos, dims)
    cuts = auto if cuts is None else [auto[a] if cuts[a] is None else cuts[a] for a in range(3)]
    steps = 2 if n == 121 else 3

    def work(sim, r):
        sim.upload_global(pos)
        out = []
        for k in range(steps):
            sim.step()
            if k == 0 and steps == 3:
                continue
            sim.output_snapshot()
            lg = sim.output_wait()
            block = sim.field(F.OUTPUT).copy()
            check_rank_list(fs, sim, lg, block)
            st = sim.output_stats()
            assert st["leaves_listed"] == lg.n_leaves and st["bytes_to_host"] == lg.n_leaves * LEAF_BYTES + HEADER_BYTES
            assert st["leaves_in_block"] == leaves_meeting(n, sim.own_lo, sim.own_hi)
            outside = sim.window_field(F.CONTAINER).copy()
            sl = tuple(slice(sim.own_lo[a] - sim.origin[a], sim.own_hi[a] - sim.origin[a]) for a in range(3))
            outside[sl] = 0
            out.append(dict(lg=lg, block=block, outside_nonzero=bool(u32(outside).any())))
        return out

    sims, res = run_group(fs, dims, n, cuts, mode, work, pos)
    _, _, _, nl = leaf_ref.geometry(n)
    for k in range(len(res[0])):
        parts = [r[k]["lg"] for r in res]
        keys = [keys_of(p.origin) for p in parts]
        count = {}
        for ks in keys:
            for o in ks:
                count[o] = count.get(o, 0) + 1
        assert max(count.values()) >= 2                     # a leaf the cut splits is listed on both sides of it
        if n == 48:
            assert max(count.values()) == 8                 # ... and the one around the corner of the eight blocks by all of them
        if mode == "replicated":
            assert all(r[k]["outside_nonzero"] for r in res)    # other ranks' sums lie around the owned block: the mask is at work
        merged = fs.merge_leaf_grids(parts)
        dense = fd.assemble(n, sims, [r[k]["block"] for r in res])
        assert np.array_equal(leaf_ref.scatter(n, merged.origin, merged.values), u32(dense))
        org, val = leaf_ref.leaf_list(dense)
        assert np.array_equal(merged.origin, org) and np.array_equal(u32(merged.values), u32(val))
        assert 0 < merged.n_leaves < nl ** 3                # strictly sparse
        assert dense.any()


def test_two_in_flight_overlap_the_next_step(fs):
    n, dims = 32, (2, 1, 1)
    pos = fs.water_cube_drop(n, 4, seed=0)
    F = fs.FIELD

    def work(sim, r):
        g = fs.LeafGridC()
        assert fs.lib.fluid_dist_output_wait(sim._h, C.byref(g)) == ERR_STATE      # nothing outstanding
        sim.upload_global(pos)
        sim.step()
        d1 = sim.field(F.OUTPUT).copy()
        sim.output_snapshot()
        sim.step()                                          # clears and refills the grid while snapshot 1 is outstanding
        d2 = sim.field(F.OUTPUT).copy()
        sim.output_snapshot()
        assert fs.lib.fluid_dist_output_snapshot(sim._h) == ERR_STATE              # a third
        assert "two output snapshots" in fs.lib.fluid_last_error().decode()
        l1, l2 = sim.output_wait(), sim.output_wait()
        check_rank_list(fs, sim, l1, d1)
        check_rank_list(fs, sim, l2, d2)
        assert fs.lib.fluid_dist_output_wait(sim._h, C.byref(g)) == ERR_STATE
        return not np.array_equal(u32(d1), u32(d2)), l1.n_leaves + l2.n_leaves

    _, res = run_group(fs, dims, n, [[0, 20, 32], [0, 32], [0, 32]], "decomposed", work, pos)
    assert any(r[0] for r in res) and all(r[1] > 0 for r in res)


def test_step_refuses_a_third_automatic_snapshot(fs):
    """One rank only: a refused rank leaves no peer inside the transport."""
    n = 32
    pos = fs.water_cube_drop(n, 4, seed=0)

    def work(sim, r):
        sim.upload_global(pos)
        sim.output_every(1)
        sim.step()
        sim.step()
        def particles():                                    # (download_local packs in no fixed order: sort by global id)
            p, _, ids = sim.download_local()
            return p[np.argsort(ids)]

        p_before = particles()
        st = fs.StepStats()
        assert fs.lib.fluid_step(sim._h, C.byref(st)) == ERR_STATE
        assert "fluid_dist_output_wait" in fs.lib.fluid_last_error().decode()
        assert np.array_equal(particles(), p_before)                   # before any work
        l1 = sim.output_wait()
        sim.step()                                          # room again
        l2, l3 = sim.output_wait(), sim.output_wait()
        check_rank_list(fs, sim, l3, sim.field(fs.FIELD.OUTPUT))
        assert l1.n_leaves and l2.n_leaves
        sim.output_every(0)
        sim.step()
        g = fs.LeafGridC()
        assert fs.lib.fluid_dist_output_wait(sim._h, C.byref(g)) == ERR_STATE      # off again: that step took none
        return True

    _, res = run_group(fs, (1, 1, 1), n, [[0, n]] * 3, "decomposed", work, pos)
    assert res == [True]


@pytest.mark.parametrize("n", [32, 121])
def test_plain_handle_gives_the_single_gpu_list(fs, n):
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 4, seed=0))
    sim.step()
    sim.step()
    h = sim._h

    def dist_snapshot():
        fs.check(fs.lib.fluid_dist_output_snapshot(h))
        g = fs.LeafGridC()
        fs.check(fs.lib.fluid_dist_output_wait(h, C.byref(g)))
        k = g.n_leaves
        assert g.n == n and k > 0
        org = np.ctypeslib.as_array(C.cast(g.origin, C.POINTER(C.c_int32)), shape=(k, 3)).copy()
        val = np.ctypeslib.as_array(C.cast(g.values, C.POINTER(C.c_float)), shape=(k, 512)).copy()
        return org, val

    a_org, a_val = dist_snapshot()
    sim.output_snapshot()
    b = sim.output_wait()
    assert a_org.tobytes() == b.origin.tobytes() and a_val.tobytes() == b.values.tobytes()
    x = [C.c_int64() for _ in range(3)]
    fs.check(fs.lib.fluid_dist_output_stats(h, *[C.byref(v) for v in x]))
    st = sim.output_stats()
    assert [v.value for v in x] == [st["leaves_in_grid"], st["leaves_listed"], st["bytes_to_host"]]
    # the two forms share the handle's two slots
    sim.output_snapshot()
    fs.check(fs.lib.fluid_dist_output_snapshot(h))
    assert fs.lib.fluid_output_snapshot(h) == ERR_STATE and fs.lib.fluid_dist_output_snapshot(h) == ERR_STATE
    c, d = sim.output_wait(), sim.output_wait()
    assert c.values.tobytes() == d.values.tobytes() == a_val.tobytes()
    # and fluid_step takes the snapshot itself on a plain handle too
    fs.check(fs.lib.fluid_dist_output_every(h, 1))
    sim.step()
    e = sim.output_wait()
    dense = sim.field(fs.FIELD.OUTPUT)
    assert np.array_equal(e.origin, leaf_ref.leaf_list(dense)[0]) and np.array_equal(u32(fs.leaves_to_dense(e)), u32(dense))
    sim.close()


@pytest.mark.parametrize("mode", ["decomposed", "replicated"])
def test_snapshots_survive_moving_cut_planes(fs, mode):
    """The scene of test_gpu_dist.py::test_cut_planes_follow_the_water with output_every(1): the grid of a step that moves the planes
    is captured from the old window (the new one's fields are zero), and a list handed out before stays readable."""
    fd = fs.load_dist()
    n, steps, dims = 64, 8, (2, 2, 2)
    pos = fs.water_cube_drop(n, 4, seed=0)
    vel = np.random.default_rng(1).standard_normal(pos.shape) * 0.3
    pos = pos + np.array([7.0, 9.0, -5.0])
    solid = np.zeros((n, n, n), dtype=np.uint8)
    solid[:2] = solid[-2:] = 1; solid[:, :2] = solid[:, -2:] = 1; solid[:, :, :2] = solid[:, :, -2:] = 1
    solid[20:30, 2:10, 24:40] = 1
    one = fs.FluidSim(n=n)
    one.set_solid(solid)
    one.upload_particles(pos, vel)
    ref = []
    for _ in range(steps):
        one.step()
        ref.append(one.field(fs.FIELD.OUTPUT).copy())
    one.close()

    def view(g):
        k = g.n_leaves
        if k == 0:
            return np.empty((0, 3), np.int32), np.empty((0, 512), np.float32)
        return (np.ctypeslib.as_array(C.cast(g.origin, C.POINTER(C.c_int32)), shape=(k, 3)),
                np.ctypeslib.as_array(C.cast(g.values, C.POINTER(C.c_float)), shape=(k, 512)))

    def work(sim, r):
        sim.set_solid(solid)
        sim.upload_global(pos, vel)
        sim.set_rebalance(4, 1.3)
        sim.output_every(1)
        out, prev, kept_over_a_move = [], None, 0
        for k in range(steps):
            own_before = (list(sim.own_lo), list(sim.own_hi))
            st = sim.step()
            g = fs.LeafGridC()
            fs.check(fs.lib.fluid_dist_output_wait(sim._h, C.byref(g)))
            o, v = view(g)                                  # the handle's own pinned memory, not a copy
            moved = bool(st["paths"] & REBALANCED)
            if prev is not None:                            # the list of step k - 1: promised until the second following snapshot
                assert np.array_equal(prev[0], prev[2]) and np.array_equal(u32(prev[1]), u32(prev[3]))
                kept_over_a_move += moved and len(prev[2]) > 0
            prev = (o, v, o.copy(), v.copy())
            out.append(dict(lg=fs.LeafGrid(g.n, o.copy(), v.copy()), moved=moved, own=own_before))
        return out, kept_over_a_move

    sims, res = run_group(fs, dims, n, fd.uniform_cuts(n, dims), mode, work, pos)
    moved = [s["moved"] for s in res[0][0]]
    assert any(moved) and all([s["moved"] for s in r[0]] == moved for r in res)     # every rank, in the same steps
    assert sum(r[1] for r in res) > 0                       # a non-empty list outlived the swap of the windows on some rank
    lo, _, l0, _ = leaf_ref.geometry(n)
    for k in range(steps):
        merged = fs.merge_leaf_grids([r[0][k]["lg"] for r in res])
        grid = fs.leaves_to_dense(merged)
        err = rel_l2(grid, ref[k])
        print(f"step {k} moved={moved[k]} leaves={merged.n_leaves} sum={grid.sum(dtype=np.float64):.6g} rel_l2={err:.3e}")
        assert grid.sum(dtype=np.float64) != 0 and err < 1e-12, (k, moved[k])
        for r in res:                                       # each rank listed the block it owned DURING the step, nothing else
            own_lo, own_hi = r[0][k]["own"]
            lgk = r[0][k]["lg"]
            d = leaf_ref.scatter(n, lgk.origin, lgk.values)
            d[tuple(slice(own_lo[a], own_hi[a]) for a in range(3))] = 0
            assert not d.any()


FLUID = os.path.join(ROOT, "fluid-simulation_amd", "fluid")


def run_fluid(fs, out, **env):
    e = fluid_env(out, 32, 4, 4, **dict({"FLUID_RAW": "1"}, **env))
    out.mkdir(exist_ok=True)
    return subprocess.run([FLUID], capture_output=True, text=True, env=e, timeout=600)


@pytest.fixture(scope="module")
def one_gpu_program(fs, tmp_path_factory):
    d = tmp_path_factory.mktemp("one")
    r = run_fluid(fs, d)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return d, r.stdout


@pytest.mark.parametrize("blocks", ["2x1x1", "2x2x2"])
def test_program_on_blocks_writes_the_same_files(fs, tmp_path, one_gpu_program, blocks):
    steps, n = 4, 32
    ref_dir, ref_out = one_gpu_program
    r = run_fluid(fs, tmp_path, FLUID_BLOCKS=blocks)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])

    def shape(text):                                        # the reference's stdout lines: the words, without the numbers
        return [ln.split("\t")[0].split(" ")[0] for ln in text.splitlines() if not ln.startswith("Time Taken")]

    assert shape(r.stdout) == shape(ref_out) and sum(ln.startswith("Iteration:") for ln in r.stdout.splitlines()) == steps
    assert r.stdout.splitlines()[-1].startswith("Time Taken")
    lo, hi = fs.grid_bounds(n)
    for i in range(steps):
        raw = open(tmp_path / f"simulation/mygrids{i}.f32", "rb").read()
        assert len(raw) == 4 + 4 * n ** 3
        dense = np.frombuffer(raw, np.float32, offset=4).reshape(n, n, n)
        _, grids = vdb_reader.read(tmp_path / f"simulation/mygrids{i}.vdb")
        assert len(grids) == 1
        assert np.array_equal(u32(grids[0].dense(lo, hi)[0]), u32(dense))
        one = np.frombuffer(open(ref_dir / f"simulation/mygrids{i}.f32", "rb").read(), np.float32, offset=4).reshape(n, n, n)
        assert dense.any() and rel_l2(dense, one) < 1e-12
    _, grids = vdb_reader.read(tmp_path / "mygrids.vdb")
    assert len(grids) == steps
    for i in range(steps):
        dense = np.frombuffer(open(tmp_path / f"simulation/mygrids{i}.f32", "rb").read(), np.float32, offset=4).reshape(n, n, n)
        assert np.array_equal(u32(grids[i].dense(lo, hi)[0]), u32(dense))


def test_program_refuses_dense_output_on_blocks(fs, tmp_path):
    r = run_fluid(fs, tmp_path, FLUID_BLOCKS="2x1x1", FLUID_OUT_DENSE="1")
    assert r.returncode != 0 and "FLUID_OUT_DENSE" in r.stderr
    assert not (tmp_path / "mygrids.vdb").exists()
    r = run_fluid(fs, tmp_path, FLUID_BLOCKS="2x1x1", FLUID_SOURCE_EVERY="2")
    assert r.returncode != 0 and "FLUID_SOURCE_EVERY" in r.stderr
