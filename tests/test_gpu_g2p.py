"""-m gpu: the one-GPU FLIPadvect phase (k_flip_delta, k_g2p / k_g2p_tiled<PIC>, the max-speed reduction, k_advect,
k_publish_dt) against tests/flip_ref.py, bit for bit.

Every scene goes through one procedure: set_solid, upload_particles, p2g, flags_index (sorts the particles, sets the solid
flags), then vel and velBefore are replaced by chosen fields and flip_advect runs.  Velocities, positions, max_speed and dt
must equal the restatement exactly, and every scene asserts which gather form it took (FLUID_PATH_G2P_TILES).  The fields
are adversarial where it matters: independent random faces everywhere, 1e3 outside W against O(1) inside, so that a
stencil read one cell off, a wrong halo at a tile seam, a swapped axis or a W mask off by one shows in the result."""
import numpy as np
import pytest

import flip_ref as fr

pytestmark = pytest.mark.gpu

P_G2P_TILES = fr.PATH_G2P_TILES


def run_phase(fs, n, solid, pos, vel, U, UB, sim=None, **kw):
    """The procedure on `sim` (a new handle with **kw if None): (sim, positions, velocities, stats)."""
    if sim is None:
        sim = fs.FluidSim(n=n, **kw)
    sim.set_solid(solid)
    sim.upload_particles(pos, vel)
    sim.p2g()
    sim.flags_index()
    sim.upload_field(fs.FIELD.VEL, U)
    sim.upload_field(fs.FIELD.VEL_BEFORE, UB)
    sim.flip_advect()
    p, v = sim.download_particles()
    return sim, p, v, sim.stats()


def check(fs, n, solid, pos, vel, U, UB, tiles, blend=1.0, nan=False, sim=None, **kw):
    """run_phase against flip_ref.flip_advect; returns (sim, restated (p, v, max_speed, dt)).  A handle passed as `sim`
    keeps the parameters it was made with: then blend must be its flip_blend and no other parameter may be given."""
    if sim is None:
        if blend < 1:
            kw["flip_blend"] = blend
    elif kw or sim.params.flip_blend != blend:
        raise ValueError("a given handle keeps its own parameters: pass its blend and nothing else")
    sim, p, v, st = run_phase(fs, n, solid, pos, vel, U, UB, sim=sim, **kw)
    prm = sim.params
    want = fr.flip_advect(n, solid, U, UB, pos, vel, blend, max_dt=prm.max_dt, dx=prm.dx)
    wp, wv, ms, dt = want
    assert bool(st["paths"] & P_G2P_TILES) == tiles, st["paths"]
    bad = ~((v == wv) | (nan & np.isnan(v) & np.isnan(wv)))
    assert not bad.any(), (bad.any(axis=1).sum(), np.flatnonzero(bad.any(axis=1))[:8])
    bad = ~((p == wp) | (nan & np.isnan(p) & np.isnan(wp)))
    assert not bad.any(), (bad.any(axis=1).sum(), np.flatnonzero(bad.any(axis=1))[:8])
    assert st["max_speed"] == ms, (st["max_speed"], ms)
    assert sim.dt == dt and st["dt_out"] == dt, (sim.dt, dt)
    return sim, want


def cube(fs, n, seed, vscale=1.0):
    pos = fs.water_cube_drop(n, 8, seed=seed)
    return pos, np.random.default_rng(seed + 100).standard_normal(pos.shape) * vscale


@pytest.mark.parametrize("blend", [1.0, 0.95, 0.0])
@pytest.mark.parametrize("n", [32, 33, 128])
def test_tiled_ragged_tiles(fs, n, blend):
    """a. Cube drops with 8 per cell: k_g2p_tiled<false> and <true>; at 128 the ~43-deep box gives z-tiles of 30 + 13 and
    partial last x / y tiles."""
    pos, vel = cube(fs, n, seed=n)
    U, UB = fr.adversarial_fields(n, np.random.default_rng(n + 1))
    check(fs, n, fr.default_solid(n), pos, vel, U, UB, tiles=True, blend=blend)


def test_tiled_with_off_grid_tail(fs):
    """b. The dense cube plus ~100 particles whose base cell is off the grid (one at 1e6): k_g2p over the n_out bucket."""
    n = 32
    rng = np.random.default_rng(2)
    lo, hi = -(n // 2), -(n // 2) + n - 1
    pos, vel = cube(fs, n, seed=3)
    off = rng.uniform(lo, hi, size=(100, 3))
    ax = rng.integers(0, 3, size=100)
    side = rng.integers(0, 2, size=100)
    off[np.arange(100), ax] = np.where(side, rng.uniform(hi + 0.6, hi + 6, 100), rng.uniform(lo - 6, lo - 0.6, 100))
    off[0] = [1e6, 0.3, -2.2]
    pos = np.concatenate([pos, off])
    vel = np.concatenate([vel, rng.standard_normal(off.shape) * 5])
    U, UB = fr.adversarial_fields(n, rng)
    for blend in (1.0, 0.95):
        check(fs, n, fr.default_solid(n), pos, vel, U, UB, tiles=True, blend=blend)


@pytest.mark.parametrize("side", ["x-", "x+", "y-", "y+", "z-", "z+"])
def test_tiled_halo_off_the_grid(fs, side):
    """c. A dense slab against one wall: base cells at indices 0 and 1 (or N-2 and N-1), the LDS halo beyond the grid edge
    and the W mask inside one tile."""
    n = 32
    rng = np.random.default_rng("xyz".index(side[0]) * 2 + (side[1] == "+"))
    a = "xyz".index(side[0])
    lo, hi = [6, 6, 6], [25, 25, 25]
    lo[a], hi[a] = (0, 5) if side[1] == "-" else (n - 6, n - 1)
    pos = fr.cells_points(fr.box_cells(lo, hi), 8, rng, -(n // 2))
    vel = rng.standard_normal(pos.shape)
    U, UB = fr.adversarial_fields(n, rng)
    for blend in (1.0, 0.95):
        check(fs, n, fr.default_solid(n), pos, vel, U, UB, tiles=True, blend=blend)


@pytest.mark.parametrize("blend", [1.0, 0.95])
def test_thread_per_particle(fs, blend):
    """d. A sparse scene over the whole grid, shell and off-grid included (< 4 per box cell): k_g2p."""
    n = 32
    rng = np.random.default_rng(4)
    lo, hi = -(n // 2), -(n // 2) + n - 1
    pos = np.concatenate([rng.uniform(lo - 2, hi + 2, size=(60000, 3)), fr.edge_particles(n, rng)[0]])
    vel = rng.standard_normal(pos.shape)
    U, UB = fr.adversarial_fields(n, rng)
    check(fs, n, fr.default_solid(n), pos, vel, U, UB, tiles=False, blend=blend)


@pytest.mark.parametrize("blend", [1.0, 0.95])
def test_advection_edges(fs, blend):
    """e. An obstacle inside W and a floating block, particles aimed at them and at the walls from all six directions
    (negative coordinates where truncation and floor differ), half-integer starting positions, the shell and past the grid.
    Ties on the moved axis: test_half_integer_ties_on_the_moved_axis."""
    n = 32
    rng = np.random.default_rng(5)
    solid = fr.obstacle_solid(n)
    pos, vel = cube(fs, n, seed=6, vscale=0.3)
    pos[:, 1] -= 4.0
    ep, ev = fr.edge_particles(n, rng)
    ap, av = fr.aimed(n, solid, rng)
    pos = np.concatenate([pos, ep, ap])
    vel = np.concatenate([vel, ev, av])
    U, UB = [f * 0.3 for f in fr.adversarial_fields(n, rng, outside=1.0)]
    sim, (wp, wv, ms, dt) = check(fs, n, solid, pos, vel, U, UB, tiles=False, blend=blend)
    k = len(pos) - len(ap)
    assert (wv[k:] == 0).sum() > 50                       # the stuck branch zeroed components
    fp, fv, _ = fr.advect(n, solid, pos, fr.gather(n, U, UB, pos, vel, blend), dt=dt, trunc=np.floor)
    assert not np.array_equal(fv, wv)                     # floor in place of truncation would show


def test_half_integer_ties_on_the_moved_axis(fs):
    """e. Moved coordinates exactly on x.5 between a fluid cell and a wall or obstacle cell, on both sides of zero (a
    power-of-two max_dt, vel == velBefore so that the gather changes no velocity): k_advect's C round (half away from
    zero) decides stuck or free where rint or floor(x + 0.5) would decide otherwise."""
    n = 32
    rng = np.random.default_rng(13)
    solid = fr.tie_solid(n)
    pos, vel, ax = fr.tie_particles(n, solid, rng)
    U = fr.adversarial_fields(n, rng)[0]
    sim, got = check(fs, n, solid, pos, vel, U, U, tiles=False, max_dt=fr.TIE_DT)
    assert got[3] == fr.TIE_DT
    t = (pos + fr.TIE_DT * vel)[np.arange(len(pos)), ax]
    assert (t - np.floor(t) == 0.5).all() and (t < 0).sum() > 100 and (t > 0).sum() > 100
    stuck = got[1][np.arange(len(pos)), ax] == 0
    assert stuck.any() and not stuck.all()
    neg, posi = fr.tie_changes(n, solid, U, pos, vel, ax, got, np.rint)
    assert neg > 0 and posi > 0, (neg, posi)
    neg, _ = fr.tie_changes(n, solid, U, pos, vel, ax, got, fr.floor_half_up)
    assert neg > 0


def test_off_grid_only_takes_no_tile(fs):
    """Every base cell off the grid: the box is empty, no tile kernel runs (the bit stays clear), k_g2p serves the bucket
    and the particles keep their velocities and move freely."""
    n = 32
    rng = np.random.default_rng(14)
    lo, hi = -(n // 2), -(n // 2) + n - 1
    pos = rng.uniform(lo, hi, size=(300, 3))
    ax = rng.integers(0, 3, size=300)
    side = rng.integers(0, 2, size=300)
    pos[np.arange(300), ax] = np.where(side, rng.uniform(hi + 0.6, hi + 6, 300), rng.uniform(lo - 6, lo - 0.6, 300))
    pos[0] = [1e6, 0.3, -2.2]
    vel = rng.standard_normal(pos.shape)
    U, UB = fr.adversarial_fields(n, rng)
    sim, got = check(fs, n, fr.default_solid(n), pos, vel, U, UB, tiles=False)
    assert np.array_equal(got[1], vel)


def test_dt_branches_and_rest(fs):
    """e. dt bounded by max_dt (slow), by dx / maxSpeed (one fast particle; dx = 1 and dx = 0.5), then everything at rest on
    the same handle right after the fast scene: maxSpeed 0 and dt = max_dt, nothing carried over."""
    n = 32
    solid = fr.default_solid(n)
    rng = np.random.default_rng(7)
    pos, vel = cube(fs, n, seed=8, vscale=0.1)
    U, UB = [f * 0.1 for f in fr.adversarial_fields(n, rng, outside=1.0)]
    sim, want = check(fs, n, solid, pos, vel, U, UB, tiles=True)
    assert want[3] == sim.params.max_dt
    fast = vel.copy()
    fast[17] = [-120.0, 45.0, 80.0]
    for dx in (1.0, 0.5):
        sim, want = check(fs, n, solid, pos, fast, U, UB, tiles=True, dx=dx)
        assert want[3] == dx / want[2] < sim.params.max_dt
    z = np.zeros_like(U)
    sim, want = check(fs, n, solid, pos, np.zeros_like(vel), z, z, tiles=True, sim=sim)
    assert want[2] == 0 and want[3] == sim.params.max_dt


def test_nan_velocity(fs):
    """e. One particle with a NaN velocity ends NaN whichever advection branch it takes and does not set dt."""
    n = 32
    solid = fr.default_solid(n)
    solid[n // 2, n // 2, n // 2] = 1                     # world (0, 0, 0)
    rng = np.random.default_rng(9)
    pos, vel = cube(fs, n, seed=10)
    pos = np.concatenate([pos, [[0.2, 0.9, -0.3]]])
    vel = np.concatenate([vel, [[np.nan] * 3]])
    U, UB = fr.adversarial_fields(n, rng)
    sim, (wp, wv, ms, dt) = check(fs, n, solid, pos, vel, U, UB, tiles=True, nan=True)
    assert np.isnan(wp[-1]).all() and np.isnan(wv[-1]).all() and np.isfinite(wp[:-1]).all()
    assert ms == fr.max_speed(wv[:-1]) > 0


def test_at_size_256(fs):
    """f. One 256^3 cube drop with 8 per cell (~5.3 M particles, 3 z-tiles) on adversarial fields."""
    n = 256
    pos, vel = cube(fs, n, seed=11)
    U, UB = fr.adversarial_fields(n, np.random.default_rng(12))
    sim, _ = check(fs, n, fr.default_solid(n), pos, vel, U, UB, tiles=True)
    sim.close()
