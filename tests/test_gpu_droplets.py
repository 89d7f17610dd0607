"""-m gpu: the droplet search (k_drop_find, k_drop_clear) and the per-droplet solve (k_drop_solve) of csrc/kernels_droplets.hip on
hand-built pockets, one scene per edge of the contract its header comment states.

Nothing here compares the kernel with itself (but the two-runs case): the claimed rows are compared with the plain labelling and the
restated contract of tests/droplet_ref.py (label, claim_rule), the pressures with the long-double true residual of
tests/pressure_system.py.  Each one-GPU case uploads CONTAINER, SOLID and a seeded random VEL, runs flags_index and one
pressure_pass with FLUID_TILE_LISTS=1 and FLUID_DROPLETS_MIN=0, and asserts

  soundness     every row of droplets() is one whole component of label, <= 64 cells, ascending, no cell or row twice; the
                droplet path bit is set exactly when a row came back; num_active still counts the claimed cells;
  completeness  the claimed components are exactly claim_rule's must-claim set (not where a slot range overflows);
  pressure      the whole system to ETA_BAR and OMEGA_BAR, every component of <= 64 cells (claimed or not) to OMEGA_BAR on its
                own, p = 0 off the unknowns, and FLUID_PATH_DROPLETS_SHORT clear — in every scene, no excuse for a short stop.

Which clause each scene pins (droplet_ref.SCENES):
  size          (c) at most 64 cells: 63 and 64 claimed, 65 not
  reach_lines   DROP_MAXSWEEPS: a line of 11 on x, y, z is claimed, a line of 12 is not
  reach_bent    DROP_MAXSWEEPS alone (small boxes): a hook of path length 10 / 11 from its tip; a "C" with two local first cells
                whose lower label needs 10 / 11 sweeps
  window        (a) closed inside the window with a free layer: cells at o+10 claimed, at o+11 not, per axis; (b) the first cell
                at the core's corners (0,0,0) and (7,7,7)
  window_low    (a) on the low side: y and z down to o-3 claimed, o-4 not (only at a larger x than the first cell's)
  neighbours    "closed": edge and corner contact and a one-cell gap separate two claims; a pocket one air cell above the pool
                is claimed, one joined to it by a face is not; a fluid cell walled in by six solids is no unknown, p = 0
  crowd         256 claims from one block: the block's numbering of its claims, one atomic per block
  overflow      slot ranges of DROP_CAP / DROP_NCTR: more pockets than DROP_CAP, more than 1 024 in a range; what does not fit
                stays in the global solve, nothing is claimed twice
  all_pockets   the global system left empty by the claims
  solids        rows with Neumann faces: on and under a shelf, at the wall, in the corner
  sealed        the solve's iteration cap: pockets cast in solid with one open face (Jacobi-scaled condition 200 - 950), over
                several right-hand sides
  grid_edge     n = 44: first cells in the last, partial core block of each axis
  decomposed    the owned-cells clause of a decomposed run (2 x 2 x 2 blocks): inside a block, window into the halo, across a cut
                plane, on the corner of three cuts
  three / none  stale slots on a reused handle, the every-8th-step search with FLUID_DROPLETS_MIN unset

Findings on the GPU are recorded in the docstrings of the tests that met them."""
import numpy as np
import pytest

import droplet_ref as dr
import pressure_system as ps

pytestmark = pytest.mark.gpu

P_LISTS, P_DROPS, P_SHORT = 2, 64, 256


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("FLUID_TILE_LISTS", "1")
    monkeypatch.setenv("FLUID_DROPLETS_MIN", "0")
    return monkeypatch


def make_sim(fs, n):
    sim = fs.FluidSim(n=n)
    assert np.array_equal(sim.field(fs.FIELD.SOLID), dr.shell_solid(n)), "the builders' wall shell is not the handle's"
    sim.upload_particles(np.zeros((0, 3)))
    return sim


def velocity(n, seed):
    return np.random.default_rng(seed).standard_normal((3, n, n, n))


def run_scene(fs, sim, name, seed=3):
    """One pass over the scene's masks.  p2g with no particles first: it zeroes the fields and the step's statistics, as at the
    start of every step."""
    c, s, notes, comps, _ = dr.built(name)
    F = fs.FIELD
    sim.p2g()
    sim.set_solid(s)
    sim.upload_field(F.CONTAINER, c)
    sim.upload_field(F.VEL, velocity(notes["n"], seed))
    sim.flags_index()
    sim.pressure_pass()
    return dict(rows=sim.droplets(), st=sim.stats(), dt=sim.dt, solid=sim.field(F.SOLID), flags=sim.field(F.FLAGS),
                indices=sim.field(F.INDICES), diver=sim.field(F.DIVER), pressure=sim.field(F.PRESSURE))


def component_omegas(sys_, res, comps, which):
    """omega of each component `which` from the rows of a whole-system residual (what pressure_system.components computes row
    set by row set: the componentwise measure is a maximum over rows)."""
    q = np.asarray(np.where(res["mag"] > 0, np.abs(res["r"]) / np.where(res["mag"] > 0, res["mag"], 1), np.where(np.abs(res["r"]) > 0, np.inf, 0)),
                   dtype=np.float64)
    cid = comps.ids[sys_.cells[res["rows"]]]
    out = np.zeros(len(comps))
    np.maximum.at(out, cid, q)
    return out[which]


def check_scene(name, got, expect_rows=None):
    """Every assertion of the module docstring on one pass.  expect_rows: None — the contract decides; 0 — the search was skipped."""
    c, s, notes, comps, _ = dr.built(name)
    n = notes["n"]
    rows, st = got["rows"], got["st"]
    assert np.array_equal(got["solid"], s)
    sys_, res = ps.check_field_solve(got["solid"], got["flags"], got["indices"], got["diver"], got["pressure"], got["dt"])
    tag = f"{name}: unknowns {sys_.size} rows {len(rows)} eta {res['eta']:.2e} omega {res['omega']:.2e} paths {st['paths']}"
    print(tag)
    # the device's unknowns are the reference's
    assert np.array_equal(np.sort(sys_.cells[sys_.in_system]), np.flatnonzero(comps.ids >= 0)), tag
    # soundness
    claimed = []
    for r in rows:
        cells = r[r >= 0]
        assert 1 <= len(cells) <= dr.POCKET_MAX and np.all(np.diff(cells) > 0) and not (r[len(cells):] >= 0).any(), (tag, r)
        k = int(comps.ids[cells[0]])
        assert k >= 0 and np.array_equal(cells, comps.cells[k]), (tag, "a row that is not one whole component", cells)
        claimed.append(k)
    assert len(set(claimed)) == len(claimed), (tag, "a component claimed twice")
    assert bool(st["paths"] & P_DROPS) == (len(rows) > 0), tag
    assert st["num_active"] == int((got["indices"] >= 0).sum()) == sys_.size, tag
    # completeness
    must = dr.claim_rule(comps, n)
    if expect_rows == 0:
        assert len(rows) == 0, tag
    elif notes["overflow"]:
        assert len(rows) <= dr.DROP_CAP and must[claimed].all(), tag
    else:
        assert set(claimed) == set(np.flatnonzero(must).tolist()), \
            (tag, "claimed but must not", sorted(set(claimed) - set(np.flatnonzero(must).tolist())),
             "must but not claimed", sorted(set(np.flatnonzero(must).tolist()) - set(claimed)))
        for p in notes["pockets"]:          # the same, said by name
            assert (int(comps.ids[p["cells"][0]]) in claimed) == p["claim"], (tag, p["name"], p["why"])
    # pressure
    assert res["eta"] <= ps.ETA_BAR and res["omega"] <= ps.OMEGA_BAR, tag
    small = np.flatnonzero(comps.sizes <= dr.POCKET_MAX)
    if len(small) <= 512:
        b, p = sys_.gather(got["diver"]), sys_.gather(got["pressure"])
        om = np.array([r["omega"] for r in ps.components(sys_, b, p, [comps.cells[k] for k in small])])
    else:
        om = component_omegas(sys_, res, comps, small)
    if len(om):
        assert om.max() <= ps.OMEGA_BAR, (tag, "component", int(small[np.argmax(om)]), float(om.max()))
    for cell in notes.get("walled", []):
        assert got["indices"].reshape(-1)[cell] >= 0 and got["pressure"].reshape(-1)[cell] == 0, tag
    assert st["paths"] & P_SHORT == 0, (tag, "a droplet's own solve stopped short of the tolerance")
    assert np.isfinite(st["relres"]), tag
    return claimed


def one_handle(fs, names, n=48, seeds=(3,)):
    sim = make_sim(fs, n)
    try:
        for name in names:
            for seed in seeds:
                check_scene(name, run_scene(fs, sim, name, seed))
    finally:
        sim.close()


def test_size(fs, env):
    one_handle(fs, ["size"])


def test_reach(fs, env):
    one_handle(fs, ["reach_lines", "reach_bent"])


def test_window(fs, env):
    one_handle(fs, ["window", "window_low"])


def test_neighbours(fs, env):
    one_handle(fs, ["neighbours"])


def test_crowd(fs, env):
    """256 single cells from one block: each p = b / diag (a one-row component's omega is |b - diag p| / (|diag p| + |b|))."""
    one_handle(fs, ["crowd"])


def test_overflow(fs, env):
    """n = 64, more pockets than slots.  Which block loses its slots depends on the order the blocks arrive in, HOW MANY are kept
    does not: every range keeps min(its claims, DROP_CAP / DROP_NCTR)."""
    name = "overflow"
    c, s, notes, comps, _ = dr.built(name)
    n = notes["n"]
    sim = make_sim(fs, n)
    try:
        got = run_scene(fs, sim, name)
        claimed = check_scene(name, got)
    finally:
        sim.close()
    x, r = np.divmod(comps.first, n * n)
    y, z = np.divmod(r, n)
    nc = n // dr.CORE
    per_range = np.bincount((((x // 8) * nc + y // 8) * nc + z // 8) % dr.DROP_NCTR, minlength=dr.DROP_NCTR)
    assert per_range.max() > dr.DROP_CAP // dr.DROP_NCTR and len(comps) > dr.DROP_CAP
    assert len(claimed) == int(np.minimum(per_range, dr.DROP_CAP // dr.DROP_NCTR).sum())
    assert got["st"]["paths"] & P_LISTS        # the pockets that found no slot are solved by the global solve


def test_everything_is_a_pocket(fs, env):
    """No pool: the claims leave the global system empty; the pass completes, relres is finite, the pressures meet the bars."""
    one_handle(fs, ["all_pockets"])


def test_solids(fs, env):
    one_handle(fs, ["solids"])


def test_sealed_pockets_converge(fs, env):
    """Pockets cast in solid with one open face, eight right-hand sides: the droplet solve must reach its stopping rule (the
    short bit stays clear) and every pocket the bars.

    Finding: with k_drop_solve's first cap of n + 8 iterations FLUID_PATH_DROPLETS_SHORT came up for seven of these eight
    right-hand sides (the pressures still met the bars: the recursive residual stood at a few 1e-16 of |b| at the cap, but the
    stopping rule was never reached, pass after pass).  The float64 restatement needs up to 2 n iterations on such pockets
    (tests/test_droplet_ref.py prints the counts); the cap is 2 n + 16 now.  The search itself met the contract in every scene
    of this module: no completeness or soundness mismatch, so claim_rule stands as the header comment states it."""
    one_handle(fs, ["sealed"], seeds=range(8))


def test_grid_edge(fs, env):
    one_handle(fs, ["grid_edge"], n=44)


SEQUENCE = ["crowd", "three", "none", "three"]


def test_reused_handle(fs, env):
    """256 claims, then three, then none, then three again on one handle: a slot of an earlier search never comes back."""
    one_handle(fs, SEQUENCE)


def test_reused_handle_searching_every_8th_step(fs, monkeypatch):
    """FLUID_DROPLETS_MIN unset: after a search that found fewer than 4 000 the next seven steps do not search.  A skipped search
    reports no droplet and no path bit, and the global solve carries the pockets to the same bars."""
    monkeypatch.setenv("FLUID_TILE_LISTS", "1")
    monkeypatch.delenv("FLUID_DROPLETS_MIN", raising=False)
    sim = make_sim(fs, 48)
    try:
        for i, name in enumerate(SEQUENCE + SEQUENCE + ["three"]):
            searched = i % 8 == 0
            check_scene(name, run_scene(fs, sim, name), expect_rows=None if searched else 0)
    finally:
        sim.close()


@pytest.mark.parametrize("name", [k for k in dr.SCENES if k not in ("overflow", dr.DECOMPOSED)])
def test_two_runs_same_bits(fs, env, name):
    """A second fresh handle gives the same pressure bit for bit: the order in which blocks and atomics ran does not reach the sums."""
    out = []
    for _ in range(2):
        sim = make_sim(fs, dr.built(name)[2]["n"])
        try:
            out.append(run_scene(fs, sim, name))
        finally:
            sim.close()
    assert np.array_equal(out[0]["pressure"], out[1]["pressure"])
    assert sorted(map(tuple, out[0]["rows"].tolist())) == sorted(map(tuple, out[1]["rows"].tolist()))


def _blocks(fs, n, pos, vel, cg, monkeypatch):
    """2 x 2 x 2 in-process blocks, one step (in the style of test_gpu_residual.run_blocks_checked): the owned blocks of the last
    pass's fields assembled, and every rank's statistics and owned box."""
    monkeypatch.setenv("FLUID_DIST_CG", cg)
    fd = fs.load_dist()
    dims = (2, 2, 2)
    grp = fd.LocalGroup(8)
    F = fs.FIELD
    fids = (F.SOLID, F.FLAGS, F.INDICES, F.DIVER, F.PRESSURE)
    sims = [None] * 8

    def work(r):
        sim = fd.DistFluidSim(n, dims, fd.uniform_cuts(n, dims), grp.comms[r], dist_solve="decomposed")
        sims[r] = sim
        sim.upload_global(pos, vel)
        st = sim.step()
        return dict(st=st, fields=[sim.field(f) for f in fids], lo=list(sim.own_lo), hi=list(sim.own_hi), info=sim.info())

    try:
        res = grp.run(work)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    arrs = []
    for f in range(len(fids)):
        a = np.zeros((n, n, n), dtype=res[0]["fields"][f].dtype)
        for r in res:
            a[r["lo"][0]:r["hi"][0], r["lo"][1]:r["hi"][1], r["lo"][2]:r["hi"][2]] = r["fields"][f]
        arrs.append(a)
    assert all(r["info"]["cg_form"] == (1 if cg == "cgear" else 0) for r in res)
    return res, arrs


@pytest.mark.parametrize("cg", ["cgear", "cg"])
def test_decomposed(fs, env, cg):
    """Pockets built from particles on cell centres (the decomposed handle takes no fields): one inside a block, two owned by one
    block with their window in the neighbour's cells, two across a cut plane, one on the corner where three cuts meet.  The
    handle exposes no droplet list: the owned-cells clause shows in the path bits — FLUID_PATH_DROPLETS exactly on the ranks for
    which claim_rule(own = the rank's cells) claims something — and in the pressures, which meet the whole-system bars and the
    per-component bar whoever solved them, and agree with the one-GPU handle on the same particles (tolerance of
    test_decomposed_with_droplets_and_galerkin_levels)."""
    from test_gpu_dist import single
    from conftest import rel_l2
    c, s, notes, comps, _ = dr.built(dr.DECOMPOSED)
    n = notes["n"]
    lo, _ = fs.grid_bounds(n)
    pos = dr.particles_on_centres(c, lo)
    vel = np.random.default_rng(12).standard_normal(pos.shape) * 0.3
    res, (solid, flags, indices, diver, pressure) = _blocks(fs, n, pos, vel, cg, env)
    dt = res[0]["st"]["dt_in"]
    assert np.array_equal(solid, s)
    sys_, r = ps.check_field_solve(solid, flags, indices, diver, pressure, dt)
    tag = f"decomposed {cg}: unknowns {sys_.size} eta {r['eta']:.2e} omega {r['omega']:.2e} paths {[q['st']['paths'] for q in res]}"
    print(tag)
    assert np.array_equal(np.sort(sys_.cells[sys_.in_system]), np.flatnonzero(comps.ids >= 0)), tag   # the particles mark the masks' cells
    assert r["eta"] <= ps.ETA_BAR and r["omega"] <= ps.OMEGA_BAR, tag
    small = np.flatnonzero(comps.sizes <= dr.POCKET_MAX)
    assert len(small) == len(notes["pockets"])
    om = [q["omega"] for q in ps.components(sys_, sys_.gather(diver), sys_.gather(pressure), [comps.cells[k] for k in small])]
    assert max(om) <= ps.OMEGA_BAR, (tag, om)
    claims = 0
    for q in res:
        own = np.zeros((n, n, n), dtype=bool)
        own[q["lo"][0]:q["hi"][0], q["lo"][1]:q["hi"][1], q["lo"][2]:q["hi"][2]] = True
        must = dr.claim_rule(comps, n, own)
        for p in notes["pockets"]:
            if not p["claim"]:
                assert not must[int(comps.ids[p["cells"][0]])], p["name"]
        claims += int(must.sum())
        assert bool(q["st"]["paths"] & P_DROPS) == bool(must.any()), (tag, q["lo"], q["hi"])
        assert q["st"]["paths"] & P_SHORT == 0, tag
    assert claims == sum(p["claim"] for p in notes["pockets"])       # each claimable pocket has exactly one owner
    ref = single(fs, n, pos, vel, 1)
    assert ref["st"][0]["paths"] & P_DROPS
    assert np.array_equal(indices, ref["indices"])
    assert rel_l2(pressure, ref["pressure"]) < 1e-7, tag
