"""-m gpu: the heads of the PCG and V-cycle kernels (partial sums re-summed by every block, the done flag, the first loads of a
tile) reorder loads only: every result stays bit for bit what the build before that change gave.

tests/golden/solver_heads.npz was recorded with that earlier build on an MI355X (record() below, the same code the tests run).
A pressure field is kept as the SHA-256 of its bytes plus every k-th cell per axis (a 104^3 field of doubles is 9 MB); both
must match exactly.

  * full tanks at four sizes chosen for the number of partial sums a block re-sums (256 threads, one value per thread and round):
      24^3   SQ tiles 6 x 3 x 1 = 18                       no second value per thread
      64^3   SQ tiles 16 x 8 x 2 = 256                     exactly one value per thread
      72^3   SQ tiles 18 x 9 x 3 = 486                     an uneven second round
      104^3  SQ tiles 26 x 13 x 4 = 1352, capped at 1024;  level-0 up leg 7 x 14 x 14 = 1372 blocks > 1024: folded by k_sum2 first
  * a mostly-air scene swept by the tile lists (XR over the row list) and by the dense forms;
  * a handle whose first batch of bodies overshoots (V-cycle, SQ and XR launches after `done` is set) against a fresh handle.
"""
import hashlib
import os

import numpy as np
import pytest

from test_gpu_parity import _shape_particles

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_heads.npz")
P_LISTS = 2
TANKS = [24, 64, 72, 104]
# (name, FLUID_TILE_LISTS, FLUID_ROW_SWEEPS).  With the lists on, the level-0 legs and SQ sweep their tile lists and XR the list of z rows
# (k_pcg_xr_rows); FLUID_ROW_SWEEPS picks the row-wise forms of the grid kernels around the solve.  k_pcg_xr_t, XR over the tile list,
# runs only when a listed box has no row with an unknown: no scene reaches it through the API.
FORMS = [("dense", "0", "0"), ("lists", "1", "0"), ("lists_rowwise", "1", "1")]


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _sub(a):
    k = max(1, a.shape[0] // 16)
    return np.ascontiguousarray(a[::k, ::k, ::k])


def _tank_particles(fs, n):
    """Two particles in every cell of the grid, seeded jitter and velocities: the active box is the whole grid."""
    lo, hi = fs.grid_bounds(n)
    rng = np.random.default_rng(100 + n)
    ax = np.arange(lo, hi + 1)
    cells = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    pos = np.repeat(cells, 2, axis=0) + rng.uniform(-0.4, 0.4, size=(len(cells) * 2, 3))
    return pos, rng.standard_normal(pos.shape) * 0.5


def _snapshot(fs, sim, st, out, key):
    p = sim.field(fs.FIELD.PRESSURE)
    out[key + "/pressure_sha"] = _sha(p)
    out[key + "/pressure_sub"] = _sub(p)
    out[key + "/cg_iters"] = np.int64(st["cg_iters"])
    out[key + "/relres"] = np.float64(st["relres"])
    out[key + "/paths"] = np.int64(st["paths"])
    out[key + "/outer_passes"] = np.int64(st["outer_passes"])


def run_tank(fs, n):
    out = {}
    sim = fs.FluidSim(n=n, solve_start="zero")
    pos, vel = _tank_particles(fs, n)
    sim.upload_particles(pos, vel)
    st = sim.step()
    _snapshot(fs, sim, st, out, f"tank{n}")
    sim.close()
    return out


def run_form(fs, name, lists, rows, setenv):
    """Three disconnected blobs in a 48^3 grid (most of the box is air), two steps."""
    setenv("FLUID_TILE_LISTS", lists)
    setenv("FLUID_ROW_SWEEPS", rows)
    out = {}
    n = 48
    rng = np.random.default_rng(5)
    pos = _shape_particles(fs, n, "blobs", rng)
    vel = rng.standard_normal(pos.shape) * 0.5
    sim = fs.FluidSim(n=n, solve_start="zero")
    sim.upload_particles(pos, vel)
    for step in range(2):
        st = sim.step()
        _snapshot(fs, sim, st, out, f"{name}/step{step}")
    p, v = sim.download_particles()
    out[f"{name}/pos_sha"] = _sha(p)
    out[f"{name}/vel_sha"] = _sha(v)
    sim.close()
    return out


def record(fs, setenv):
    """Everything the fixture holds, computed by the build that `fs` is."""
    out = {}
    for n in TANKS:
        out.update(run_tank(fs, n))
    for name, lists, rows in FORMS:
        out.update(run_form(fs, name, lists, rows, setenv))
    return out


def _compare(got, gold):
    assert got, "nothing computed"
    for k, v in got.items():
        assert k in gold.files, k
        print(k, "equal" if np.array_equal(v, gold[k]) else f"DIFFERS: {v if np.ndim(v) == 0 else ''} / {gold[k] if np.ndim(v) == 0 else ''}")
    for k, v in got.items():
        assert np.array_equal(v, gold[k]), k


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("n", TANKS)
def test_full_tank_bit_identical(fs, gold, n):
    got = run_tank(fs, n)
    assert got[f"tank{n}/cg_iters"] >= 3     # a real solve, several bodies
    _compare(got, gold)


@pytest.mark.parametrize("name,lists,rows", FORMS)
def test_list_and_dense_forms_bit_identical(fs, gold, name, lists, rows, monkeypatch):
    got = run_form(fs, name, lists, rows, monkeypatch.setenv)
    for step in range(2):
        assert bool(got[f"{name}/step{step}/paths"] & P_LISTS) == (lists == "1")
    _compare(got, gold)


def _hard_scene(fs, n):
    return _tank_particles(fs, n)                     # one pass of about 40 bodies (the tanks above: 40 .. 48)


def _easy_scene(fs, n):
    rng = np.random.default_rng(5)
    pos = _shape_particles(fs, n, "needle", rng)      # one pass of 16 bodies
    return pos, rng.standard_normal(pos.shape) * 0.5


def test_finished_solve_is_left_alone(fs, monkeypatch):
    """Handle B steps a scene whose solves need more bodies than the next scene's, so the first batch of B's second step (as many
    bodies as its last solve needed, unpolled) runs V-cycle, SQ and XR launches after `done` is set.  They must change nothing:
    the step is bit for bit the step of a fresh handle A."""
    monkeypatch.setenv("FLUID_TILE_LISTS", "0")
    n = 48
    F = fs.FIELD
    hard, hard_v = _hard_scene(fs, n)
    easy, easy_v = _easy_scene(fs, n)

    a = fs.FluidSim(n=n, solve_start="zero")
    dt0 = a.dt
    a.upload_particles(easy, easy_v)
    sa = a.step()
    pa, va = a.download_particles()
    pra = a.field(F.PRESSURE)
    a.close()

    b = fs.FluidSim(n=n, solve_start="zero")
    b.upload_particles(hard, hard_v)
    sh = b.step()
    b.upload_particles(easy, easy_v)
    b.dt = dt0
    sb = b.step()
    pb, vb = b.download_particles()
    prb = b.field(F.PRESSURE)
    b.close()

    print(f"hard: passes {sh['outer_passes']} iters {sh['cg_iters']} last {sh['cg_iters_last']} | easy: passes {sa['outer_passes']} iters {sa['cg_iters']} "
          f"last {sa['cg_iters_last']}")
    # the first batch of a pass runs the bodies that the same pass of the step before needed, + 1: the hard scene's first pass needs more
    assert sh["outer_passes"] == 1 and sa["outer_passes"] == 1 and sh["cg_iters"] >= sa["cg_iters"] + 3, (sh, sa)
    assert sb["cg_iters"] == sa["cg_iters"] and sb["outer_passes"] == sa["outer_passes"] and sb["paths"] == sa["paths"]
    assert sb["relres"] == sa["relres"]
    assert np.array_equal(prb, pra)
    assert np.array_equal(pb, pa)
    assert np.array_equal(vb, va)
