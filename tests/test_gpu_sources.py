"""-m gpu: particle sources and sinks of the one-GPU step (include/fluid_hip.h, "particle sources and sinks").

fluid_add_particles against the oracle run on the same union set, its vel == NULL form (interpFromGrid) against the numpy
clampedCatmullRom (tests/sources_ref.py), the reference's switched-on emitter (fluid.cc:1374-1375, 1495-1497) against the oracle,
ADD / FILL sources and sinks against their restatements, and a steady inflow/outflow run judged by the true residual of its
last pressure solve (tests/pressure_system.py)."""
import ctypes as C

import numpy as np
import pytest

import pressure_system as ps
import sources_ref as sr
from conftest import rel_l2
from sources_ref import base_cells, default_solid

pytestmark = pytest.mark.gpu

TOL_F = 1e-4      # the parity tolerance of tests/test_gpu_parity.py
P_SOURCES = 512


def test_append_matches_the_oracle_on_the_union(fs, oracle):
    n = 24
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim, orc = fs.FluidSim(n=n), oracle.Oracle(n=n)
    sim.upload_particles(pos)
    orc.set_particles(pos)
    sim.step(); orc.step()
    p0, v0 = sim.download_particles()
    rng = np.random.default_rng(3)
    new = rng.uniform(-6, 6, size=(500, 3))
    newv = rng.standard_normal((500, 3))
    sim.add_particles(new, newv)
    p1, v1 = sim.download_particles()
    assert sim.num_particles == len(pos) + 500
    assert np.array_equal(p1[:len(pos)], p0) and np.array_equal(v1[:len(pos)], v0)
    assert np.array_equal(p1[len(pos):], new) and np.array_equal(v1[len(pos):], newv)
    po, vo = orc.particles()
    orc.set_particles(np.concatenate([po, new]), np.concatenate([vo, newv]))
    for i in range(2):
        sg, so = sim.step(), orc.step()
        assert sg["num_active"] == so["num_active"] and sg["outer_passes"] == so["outer_passes"], (i, sg, so)
        assert np.array_equal(sim.field(fs.FIELD.INDICES), orc.field(4))
        p, v = sim.download_particles(); po, vo = orc.particles()
        assert rel_l2(p, po) < TOL_F and rel_l2(v, vo) < TOL_F, (i, rel_l2(p, po), rel_l2(v, vo))


def test_interp_from_grid(fs):
    n = 24
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim = fs.FluidSim(n=n)
    solid = default_solid(n)
    solid[12:15, 3:5, 12:15] = 1    # an obstacle under the cube
    sim.set_solid(solid)
    sim.upload_particles(pos)
    with pytest.raises(fs.FluidError) as e:
        sim.add_particles(np.zeros((3, 3)))
    assert e.value.code == 3
    for _ in range(3):
        sim.step()
    lo, hi = sim.lo, sim.hi
    rng = np.random.default_rng(5)
    pts = [rng.uniform(-5, 5, size=(400, 3)),                        # in and around the water
           rng.uniform(lo + 1.4, lo + 3.6, size=(100, 3)),           # near the walls, partly outside W
           np.array([[0.0, -8.6, 0.0], [1.2, -8.1, 2.3], [0.49, -7.51, 0.5]]),   # near the obstacle (index 12..14, 3..4)
           np.array([[lo - 0.3, 0, 0], [hi + 0.2, hi, hi], [lo + 0.5, lo + 0.5, lo + 0.5], [1e6, 0, 0]])]   # outside W / the grid
    new = np.concatenate(pts)
    n0 = sim.num_particles
    vel = sim.field(fs.FIELD.VEL)
    sim.add_particles(new)
    _, v = sim.download_particles()
    got = v[n0:]
    want = sr.clamped_catmull_rom(n, vel, new)
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want), np.abs(got - want).max()    # the kernel's cell order and association: bit for bit
    assert (got[-2:] == 0).all() and (want[-1] == 0).all()


def scaled_box(n):
    m = int(round(n * 41 / 121))
    c0 = -(m // 2)
    return [c0] * 3, [c0 + m - 1] * 3


@pytest.mark.parametrize("n", [32, 48])
def test_reference_emitter_switched_on(fs, oracle, n):
    """fluid.cc:1374-1375, 1495, 1497 with the `i % 5` gate of :1379 as every = 2: the scatter with mt19937(i + 1) over the
    scaled initial box, velocities from interpFromGrid; the oracle takes the same points with the numpy clampedCatmullRom of
    its own grid."""
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim, orc = fs.FluidSim(n=n), oracle.Oracle(n=n)
    sim.upload_particles(pos)
    orc.set_particles(pos)
    lo, hi = scaled_box(n)
    bound = sim.hi
    for i in range(6):
        sg, so = sim.step(), orc.step()
        assert sg["num_active"] == so["num_active"] and sg["outer_passes"] == so["outer_passes"], (i, sg, so)
        assert np.array_equal(sim.field(fs.FIELD.INDICES), orc.field(4)), i
        if i % 2 == 0:
            new = fs.reference_scatter(lo, hi, 10.0, seed=i + 1, boundary=bound)
            sim.add_particles(new)
            po, vo = orc.particles()
            nv = sr.clamped_catmull_rom(n, orc.field(2), new)
            orc.set_particles(np.concatenate([po, new]), np.concatenate([vo, nv]))
        p, v = sim.download_particles(); po, vo = orc.particles()
        assert len(p) == len(po)
        assert rel_l2(p, po) < TOL_F and rel_l2(v, vo) < TOL_F, (i, rel_l2(p, po), rel_l2(v, vo))
    assert sim.num_particles > len(pos)


def test_add_source_restated_bit_for_bit(fs):
    n = 24
    pos = fs.water_cube_drop(n, 2, seed=1)
    solid = default_solid(n)
    solid[4, 19, 5] = 1                               # a solid cell inside the box
    lo, hi = (0, 17, 3), (6, 21, 9)                   # reaches outside W on x
    out = []
    for _ in range(2):
        sim = fs.FluidSim(n=n)
        sim.set_solid(solid)
        sim.upload_particles(pos)
        sim.set_source(0, lo, hi, 5, mode="add", every=1, vel=(0.5, -1.0, 0.25), seed=42)
        st = sim.step()
        assert st["paths"] & P_SOURCES
        ss = sim.source_stats()
        p, v = sim.download_particles()
        out.append((p, v, ss))
        sim.close()
    (p, v, ss), (p2, v2, _) = out
    assert p.tobytes() == p2.tobytes() and v.tobytes() == v2.tobytes()
    want = sr.source_points(n, 42, 0, lo, hi, 5, solid)
    n0 = len(pos)
    assert ss["emitted_last"] == len(want) == len(p) - n0 and ss["emitted_total"] == len(want)
    assert np.array_equal(p[n0:], want)
    assert (v[n0:] == [0.5, -1.0, 0.25]).all()
    c = base_cells(n, p[n0:])
    assert (c >= 2).all() and (c <= n - 3).all() and not solid[c[:, 0], c[:, 1], c[:, 2]].any()
    assert (c >= lo).all() and (c <= hi).all()
    # every = 2: nothing at step 1, then step 2 again (t = 2 feeds the hash)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    sim.set_source(3, lo, hi, 2, every=2, vel=(0, 0, 0), seed=9)
    for t in range(3):
        sim.step()
        e = sim.source_stats()["emitted_last"]
        assert (e > 0) == (t % 2 == 0), (t, e)
    p, _ = sim.download_particles()
    assert np.array_equal(p[-e:], sr.source_points(n, 9, 2, lo, hi, 2, default_solid(n)))


def test_fill_source(fs):
    n, pc = 24, 3
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    sim.step()
    lo, hi = (9, 12, 9), (14, 19, 14)                 # half in the falling cube (y 8..15), half above it
    sim.set_source(1, lo, hi, pc, mode="fill", seed=77)    # vel from the grid
    sim.step()
    vel = sim.field(fs.FIELD.VEL)                      # the grid the source read: this step's, until the next P2G
    ss = sim.source_stats()
    p, v = sim.download_particles()
    n0 = len(pos)
    old = p[:n0]
    hist = sr.base_cell_counts(n, lo, hi, old)
    want = sr.source_points(n, 77, 1, lo, hi, pc, default_solid(n), hist)
    assert ss["emitted_last"] == len(want) == len(p) - n0 > 0
    assert np.array_equal(p[n0:], want)
    after = sr.base_cell_counts(n, lo, hi, p)
    assert (after >= pc).all()                        # every box cell lies inside W here
    assert (after[hist >= pc] == hist[hist >= pc]).all() and (hist >= pc).any()
    want_v = sr.clamped_catmull_rom(n, vel, p[n0:])
    assert np.abs(want_v).max() > 0
    assert np.array_equal(v[n0:], want_v), np.abs(v[n0:] - want_v).max()


def test_add_source_grid_velocity_over_many_scan_chunks(fs):
    """An ADD source with grid velocities over 21 x 20 x 19 = 7980 cells (three scan chunks of 2048 and a ragged fourth)
    after a few steps: points and velocities restated bit for bit."""
    n, pc, seed = 48, 3, 2024
    pos = fs.water_cube_drop(n, 4, seed=5)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    for _ in range(3):
        sim.step()
    lo, hi = (10, 14, 12), (30, 33, 30)               # in and above the falling cube, negative and positive coordinates
    assert np.prod(np.array(hi) - lo + 1) == 7980
    sim.set_source(2, lo, hi, pc, mode="add", seed=seed)
    n0 = sim.num_particles
    sim.step()
    vel = sim.field(fs.FIELD.VEL)
    ss = sim.source_stats()
    p, v = sim.download_particles()
    want = sr.source_points(n, seed, 3, lo, hi, pc, default_solid(n))
    assert ss["emitted_last"] == len(want) == len(p) - n0 > 3 * 2048
    assert np.array_equal(p[n0:], want)
    want_v = sr.clamped_catmull_rom(n, vel, want)
    assert np.abs(want_v).max() > 0
    assert np.array_equal(v[n0:], want_v), np.abs(v[n0:] - want_v).max()


def test_fill_source_every_branch_of_the_plan(fs):
    """One FILL source with grid velocities whose box reaches outside W on two sides (x = 0, 1 and y = 1), holds two user solid
    cells and meets the water, with extents 11 x 10 x 11 (no stride of the grid or of a block divides them), at t = 2: the solid
    bytes come through the strided view, the histogram, the W test and the gather all take part."""
    n, pc, seed = 24, 3, 7
    lo, hi = (0, 1, 3), (10, 10, 13)                  # the cube covers the indices 8..15
    solid = default_solid(n)
    solid[4, 5, 6] = solid[3, 2, 12] = 1
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim = fs.FluidSim(n=n)
    sim.set_solid(solid)
    sim.upload_particles(pos)
    sim.step(); sim.step()
    sim.set_source(0, lo, hi, pc, mode="fill", seed=seed)    # vel from the grid
    sim.step()                                        # t = 2
    vel = sim.field(fs.FIELD.VEL)
    ss = sim.source_stats()
    p, v = sim.download_particles()
    n0 = len(pos)
    hist = sr.base_cell_counts(n, lo, hi, p[:n0])
    assert hist.max() >= pc and hist.min() == 0
    want = sr.source_points(n, seed, 2, lo, hi, pc, solid, hist)
    assert 0 < len(want) < len(sr.source_points(n, seed, 2, lo, hi, pc, default_solid(n)))   # the solid cells and the water took their share
    assert ss["emitted_last"] == len(want) == len(p) - n0
    assert np.array_equal(p[n0:], want)
    c = base_cells(n, p[n0:])
    assert (c >= 2).all() and not solid[c[:, 0], c[:, 1], c[:, 2]].any()
    want_v = sr.clamped_catmull_rom(n, vel, want)
    assert np.abs(want_v).max() > 0
    assert np.array_equal(v[n0:], want_v), np.abs(v[n0:] - want_v).max()


def test_one_gpu_and_one_block_bit_for_bit(fs):
    """The same three steps with an ADD source (grid velocities) and a FILL source (fixed velocity), no sink (sinks renumber on
    one GPU only), on a one-GPU handle and on a (1, 1, 1) decomposed handle: sorted by id, the same bytes.
    (tests/test_gpu_dist_sources.py::test_whole_run_against_one_gpu[(32, (1, 1, 1))] has a sink and compares to a tolerance.)"""
    fd = fs.load_dist()
    n, steps = 32, 3
    pos = fs.water_cube_drop(n, 4, seed=0)            # the cube covers the indices 11..21
    slots = [(0, dict(lo=(14, 23, 14), hi=(18, 24, 18), per_cell=2, mode="add", every=2, vel=None, seed=21)),          # above the cube
             (3, dict(lo=(14, 20, 14), hi=(18, 21, 18), per_cell=6, mode="fill", every=1, vel=(0.0, -2.0, 0.5), seed=22))]  # its top
    one = fs.FluidSim(n=n)
    one.upload_particles(pos)
    grp = fd.LocalGroup(1)
    blk = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    blk.upload_global(pos)
    try:
        for sim in (one, blk):
            for slot, kw in slots:
                sim.set_source(slot, **kw)
        for t in range(steps):
            one.step(); blk.step()
            assert one.source_stats() == blk.source_stats(), t
        ss = one.source_stats()
        assert ss["emitted_total"] > ss["emitted_last"] > 0
        p1, v1 = one.download_particles()             # pids are 0..np-1 in this order: no sink, nothing renumbered
        p2, v2, ids = blk.download_local()
        o = np.argsort(ids, kind="stable")
        assert np.array_equal(ids[o], np.arange(len(p1)))
        assert p2[o].tobytes() == p1.tobytes(), np.abs(p2[o] - p1).max()
        assert v2[o].tobytes() == v1.tobytes(), np.abs(v2[o] - v1).max()
    finally:
        one.close(); blk.close(); grp.close()


def test_sink(fs):
    n = 24
    pos = fs.water_cube_drop(n, 4, seed=2)
    sims = [fs.FluidSim(n=n) for _ in range(3)]
    for s in sims:
        s.upload_particles(pos)
    lo, hi = (8, 9, 8), (12, 12, 16)                  # cuts through the cube
    sims[1].set_sink(0, lo, hi)
    sims[2].set_sink(5, (3, 3, 3), (5, 5, 5))         # empty corner
    st = [s.step() for s in sims]
    (pa, va), (pb, vb), (pc, vc) = [s.download_particles() for s in sims]
    c = base_cells(n, pa)
    gone = np.all((c >= lo) & (c <= hi), axis=1)
    assert gone.any() and not gone.all()
    assert sims[1].num_particles == (~gone).sum()
    assert np.array_equal(pb, pa[~gone]) and np.array_equal(vb, va[~gone])
    assert sims[1].source_stats()["removed_last"] == gone.sum()
    assert st[1]["paths"] & P_SOURCES and not st[2]["paths"] & P_SOURCES
    assert pc.tobytes() == pa.tobytes() and vc.tobytes() == va.tobytes()
    # the survivors go on stepping; clearing the sink stops it
    sims[1].clear_sink(0)
    sims[1].step()
    assert sims[1].num_particles == (~gone).sum() and sims[1].source_stats()["removed_last"] == 0


def test_source_outside_w_changes_nothing(fs):
    n = 24
    pos = fs.water_cube_drop(n, 4, seed=0)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    a.upload_particles(pos)
    b.upload_particles(pos)
    b.set_source(0, (0, 0, 0), (1, n - 1, n - 1), 8, mode="fill")   # x = 0, 1: outside W, nothing eligible
    b.set_sink(0, (0, 0, 0), (n - 1, 1, n - 1))                       # y = 0, 1: nothing reaches it
    for i in range(10):
        sa, sb = a.step(), b.step()
        assert sa == sb, i
    for x, y in zip(a.download_particles(), b.download_particles()):
        assert x.tobytes() == y.tobytes()
    for f in (fs.FIELD.VEL, fs.FIELD.PRESSURE, fs.FIELD.INDICES):
        assert a.field(f).tobytes() == b.field(f).tobytes()
    assert b.source_stats()["emitted_total"] == 0 and b.source_stats()["removed_total"] == 0


def test_growth_keeps_the_particles(fs):
    n = 24
    pos = fs.water_cube_drop(n, 1, seed=0)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    a.upload_particles(pos)
    b.upload_particles(pos)
    b.set_source(0, (4, 4, 4), (19, 19, 19), 6, seed=1, vel=(0, 0, 0))   # far more than the upload's capacity
    a.step(); b.step()
    (pa, va), (pb, vb) = a.download_particles(), b.download_particles()
    assert len(pb) > 10 * len(pa)
    assert pb[:len(pa)].tobytes() == pa.tobytes() and vb[:len(pa)].tobytes() == va.tobytes()
    # and through fluid_add_particles
    more = np.random.default_rng(0).uniform(-8, 8, size=(4 * len(pb), 3))
    b.add_particles(more, np.zeros_like(more))
    pc, vc = b.download_particles()
    assert pc[:len(pb)].tobytes() == pb.tobytes() and vc[:len(pb)].tobytes() == vb.tobytes()
    assert np.array_equal(pc[len(pb):], more)
    b.step()


def test_steady_inflow_and_outflow_128(fs):
    n = 128
    pos = fs.water_cube_drop(n, 4, seed=0)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    src_lo, src_hi = (54, 112, 54), (73, 116, 73)
    sim.set_source(0, src_lo, src_hi, 4, mode="fill", every=2, seed=3)
    sim.set_sink(0, (2, 2, 2), (n - 3, 4, n - 3))
    box_cap = 20 * 5 * 20 * 4
    n_prev = len(pos)
    for i in range(150):
        st = sim.step()                               # raises unless FLUID_OK
        ss = sim.source_stats()
        assert sim.num_particles == n_prev + ss["emitted_last"] - ss["removed_last"], i
        assert ss["emitted_last"] <= box_cap and (i % 2 == 0 or ss["emitted_last"] == 0), (i, ss)
        n_prev = sim.num_particles
    assert n_prev <= len(pos) + 75 * box_cap
    assert ss["emitted_total"] > 0 and ss["removed_total"] > 0
    assert sim.num_particles == len(pos) + ss["emitted_total"] - ss["removed_total"]
    F = fs.FIELD
    _, res = ps.check_field_solve(sim.field(F.SOLID), sim.field(F.FLAGS), sim.field(F.INDICES), sim.field(F.DIVER),
                                  sim.field(F.PRESSURE), st["dt_in"])
    print(f"128^3 inflow/outflow: {sim.num_particles} particles, emitted {ss['emitted_total']} removed {ss['removed_total']}, "
          f"eta {res['eta']:.2e}")
    assert res["eta"] <= ps.ETA_BAR


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    h = sim._h
    src = fs.Source()
    src.lo[:] = [4, 4, 4]; src.hi[:] = [6, 6, 6]
    src.per_cell, src.every = 1, 1
    l3, h3 = (C.c_int32 * 3)(4, 4, 4), (C.c_int32 * 3)(6, 6, 6)
    pts = np.zeros((1, 3))
    x = C.c_int64()
    assert fs.lib.fluid_add_particles(h, 1, pts.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p)) == 3
    assert fs.lib.fluid_set_source(h, 0, C.byref(src)) == 3
    assert fs.lib.fluid_set_sink(h, 0, l3, h3) == 3
    assert fs.lib.fluid_get_source_stats(h, C.byref(x), None, None, None) == 3
    assert "single-GPU" in fs.lib.fluid_last_error().decode()
    sim.close()
