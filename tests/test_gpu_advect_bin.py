"""-m gpu: the step with FLUID_ADVECT_BIN / FLUID_SOLVE_TAIL on against the same step with both off.

On (the default) FLIPadvect's kernel bins the positions it writes, so that the next sort starts at its scan without a pass
over the positions and without a read-back, and the first poll of a multigrid PCG solve carries the rest of the pressure
pass behind the solve's done flag.  Off is the launch sequence without either.  Neither may change one bit of what a step
computes: every case below runs the same scene on two handles and compares particle positions, velocities, the pressure
field and every entry of the step's stats with np.array_equal / ==, step by step.  The cases where the binning must step
aside (re-upload, sources and sinks, resample, the phase API, particles off the grid, a particle that leaves the +-3 plane
window of the guess, an empty set) are each run the same way."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("FLUID_ADVECT_BIN", "FLUID_SOLVE_TAIL")


def make_sim(fs, bin_on, tail_on, **kw):
    """A handle created under the given switch settings (the library reads them once, in fluid_create)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ["FLUID_ADVECT_BIN"] = "1" if bin_on else "0"
    os.environ["FLUID_SOLVE_TAIL"] = "1" if tail_on else "0"
    try:
        return fs.FluidSim(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same_stats(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, float) and math.isnan(x):
            assert isinstance(y, float) and math.isnan(y), (k, x, y)
        else:
            assert x == y, (k, x, y)


def snapshot(fs, sim):
    p, v = sim.download_particles()
    return p, v, sim.field(fs.FIELD.PRESSURE)


def same_state(fs, a, b, where):
    pa, va, qa = snapshot(fs, a)
    pb, vb, qb = snapshot(fs, b)
    assert pa.shape == pb.shape, where
    assert np.array_equal(pa, pb, equal_nan=True), where
    assert np.array_equal(va, vb, equal_nan=True), where
    assert np.array_equal(qa, qb, equal_nan=True), where


def run_pair(fs, on, off, steps, between=None):
    """`steps` steps on both handles, everything compared after each; between(sim, i) runs on both after step i."""
    hist = []
    for i in range(steps):
        s_on, s_off = on.step(), off.step()
        same_stats(s_on, s_off)
        same_state(fs, on, off, i)
        hist.append(s_on)
        if between is not None:
            between(on, i)
            between(off, i)
    return hist


def pair(fs, pos, vel=None, modes=((True, True),), **kw):
    """One handle per switch setting in `modes` and the switch-off handle, all holding the same particles."""
    sims = [make_sim(fs, b, t, **kw) for b, t in modes] + [make_sim(fs, False, False, **kw)]
    for s in sims:
        s.upload_particles(pos, vel)
    return sims


@pytest.mark.parametrize("mode", [(True, True), (True, False), (False, True)], ids=["both", "bin", "tail"])
def test_drop_through_free_fall_into_the_splash(fs, mode):
    n = 64
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=0), modes=(mode,), n=n)
    hist = run_pair(fs, on, off, 70)
    boxes = {(tuple(h["box_lo"]), tuple(h["box_hi"])) for h in hist}
    assert len(boxes) > 10                                  # the active box moves with the water
    assert max(h["outer_passes"] for h in hist) > 1         # steps of more than one pressure pass are in the run
    assert hist[-1]["box_lo"][1] <= 2                       # ... and it ends on the floor


def test_pic_flip_blend(fs):
    n = 32
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=1), n=n, flip_blend=0.95)
    run_pair(fs, on, off, 25)


def test_solves_ended_by_the_iteration_cap(fs):
    n = 32
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=2), n=n, cg_max_iters=3, max_outer_passes=3)
    hist = run_pair(fs, on, off, 12)
    # a solve either has nothing to do (b = 0: no iteration) or runs into the cap, and most do the latter
    its = [(h["cg_iters"], h["outer_passes"]) for h in hist]
    assert all(c % 3 == 0 and c <= 3 * k for c, k in its), its
    assert sum(c == 3 * k for c, k in its) >= 8, its
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=2), n=n, cg_max_iters=8)   # some solves finish, some are cut
    run_pair(fs, on, off, 12)


def test_reupload_between_steps(fs):
    n = 32
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=3), n=n)

    def reupload(sim, i):
        if i in (2, 3, 6):
            p, v = sim.download_particles()
            sim.upload_particles(p[::-1].copy(), v[::-1].copy())
    run_pair(fs, on, off, 10, reupload)


def test_active_source_and_sink(fs):
    n = 32
    sims = pair(fs, fs.water_cube_drop(n, 4, seed=4), n=n)
    for s in sims:
        s.set_source(0, [20, 20, 12], [23, 22, 18], per_cell=2, mode="add", every=2, vel=(0.0, -3.0, 0.0), seed=7)
        s.set_sink(0, [2, 2, 2], [29, 4, 29])

    def switch_off(sim, i):   # the last steps run without either again: the binning comes back
        if i == 11:
            sim.clear_source(0)
            sim.clear_sink(0)
    hist = run_pair(fs, sims[0], sims[1], 16, switch_off)
    assert sims[0].source_stats() == sims[1].source_stats()
    assert sims[0].source_stats()["emitted_total"] > 0
    assert len(hist) == 16


def test_add_particles_between_steps(fs):
    n = 32
    on, off = pair(fs, fs.water_cube_drop(n, 4, seed=5), n=n)
    new = np.random.default_rng(11).uniform(-4, 4, size=(300, 3)) + np.array([0.0, 9.0, 0.0])

    def add(sim, i):
        if i in (1, 4):
            sim.add_particles(new + i, np.zeros_like(new))
    run_pair(fs, on, off, 8, add)


def test_resample_between_steps(fs):
    n = 32
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=6), n=n)
    parked = []

    def resample(sim, i):
        if i in (1, 5):
            parked.append(sim.resample(5))
    run_pair(fs, on, off, 9, resample)
    assert parked[0] == parked[1] and parked[2] == parked[3] and parked[0] > 0


def test_phase_api_sequence(fs):
    n = 32
    on, off = pair(fs, fs.water_cube_drop(n, 8, seed=7), n=n)
    for i in range(8):
        for s in (on, off):
            s.p2g()
            s.flags_index()
            if i % 2 == 0:
                for _ in range(2):
                    s.pressure_pass()
            else:   # the single phases: no pass-level shortcut may show through them
                s.rhs_div(0)
                s.solve()
                s.vel_update()
                s.rhs_div(1)
            s.flip_advect()
        same_stats(on.stats(), off.stats())
        same_state(fs, on, off, i)
    # and the mixed use: whole steps after phases, phases after whole steps
    run_pair(fs, on, off, 3)
    for s in (on, off):
        s.p2g()
        s.p2g()          # a second sort of the same positions
        s.flags_index()
        s.pressure_pass()
        s.flip_advect()
    same_state(fs, on, off, "mixed")
    run_pair(fs, on, off, 2)


def test_particles_off_the_grid(fs):
    n = 32
    pos = fs.water_cube_drop(n, 8, seed=8)
    hi = n // 2
    out = np.array([[hi + 5.0, 0.0, 0.0], [0.0, hi + 9.5, 1.0], [-hi - 7.0, -hi - 7.0, 3.0], [1.0, 2.0, hi + 40.0]])
    pos = np.concatenate([pos[:1000], out, pos[1000:]])
    on, off = pair(fs, pos, n=n)
    run_pair(fs, on, off, 10)
    p, _ = on.download_particles()
    assert np.array_equal(p[1000:1004], out)     # nothing reaches them


def test_a_particle_that_leaves_the_plane_window(fs):
    """dx = 4 lets the fastest particle move 4 cells in one step (dt = dx / max speed, positions in cells): one particle at the
    +x face of the water with a large +x velocity ends more than 3 planes past the box the window was guessed from, so the
    guess fails and the sort runs over the whole grid."""
    n = 48
    pos = fs.water_cube_drop(n, 4, seed=9)
    vel = np.zeros_like(pos)
    k = int(np.argmax(pos[:, 0]))
    vel[k] = [60.0, 0.0, 0.0]
    on, off = pair(fs, pos, vel, n=n, dx=4.0, max_dt=1.0)
    top = [np.round(pos[:, 0]).max()]

    def track(sim, i):
        if sim is on:
            top.append(np.round(sim.download_particles()[0][:, 0]).max())
    run_pair(fs, on, off, 5, track)
    jumps = np.diff(top)
    assert (jumps[1:] >= 4).any(), top    # a step after the first (the first sort has no guess) took it past the +-3 planes


def test_empty_particle_set(fs):
    n = 24
    on, off = pair(fs, np.zeros((0, 3)), n=n)
    run_pair(fs, on, off, 3)
    # ... and a set that a sink empties during the run
    on, off = pair(fs, fs.water_cube_drop(n, 2, seed=10), n=n)
    for s in (on, off):
        s.set_sink(0, [0, 0, 0], [n - 1, n - 1, n - 1])
    run_pair(fs, on, off, 3)
    assert on.num_particles == 0
