"""-m gpu: particle -> grid on the device, every cell against the exact sums of tests/p2g_ref.py.

For every case: sim.p2g(); sim.flags_index(), then for EVERY cell
  1. numerator bar   |VEL * double(CONTAINER) - N| <= gamma(k + 4, 2^-53) T      (~k * 1e-16: one lost or repeated addend fails it)
  2. weight, reference bar   |w - Wp| <= gamma(k, 2^-24) A                         (any legal form)
  3. weight, project bar     |w - Wp| <= (m 2^-24 + (k + 2) 2^-53) A               (double partials narrowed m times: m = 3 for the
     row and crowd forms (one per source x-plane, k_p2g_combine), m = 27 for the tile form (one per source cell: 9 rows x 3 z
     sources, "one rounding per source cell", k_p2g_tiles))
  4. exact facts: INDICES, num_active and the flag bits equal the oracle's; VEL_BEFORE is VEL and WEIGHTS is CONTAINER bit for bit;
     solid cells and cells outside the reference's support hold exactly 0 (stale partials, uncleared boxes)
  5. the form that ran, through stats()["paths"].
The serial oracle is used for the integer facts only; every float is held to the exact reference.

The VEC = false instantiation of k_p2g_rows cannot be reached through a one-GPU handle (particle capacities are even and the
arrays 16 B aligned by construction; only a decomposed run's shifted ghost ranges take it), so no case here depends on it.
"""
import time

import numpy as np
import pytest

import p2g_ref as R
import p2g_scenes as S

pytestmark = pytest.mark.gpu

TILES, CROWD = 1, 16                       # FLUID_PATH_P2G_TILES, FLUID_PATH_P2G_CROWD
NARROWINGS = {"rows": 3, "crowd": 3, "tiles": 27}
FORMS = ("rows", "crowd", "tiles", None)   # None: FLUID_P2G_FORM unset, the host's own choice
RATIOS = {}                                # form -> what -> largest error / bar seen in this session (printed after the module)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    """After the module: the largest error / bar ratios seen per form, for the record."""
    yield
    for form, r in sorted(RATIOS.items()):
        print(f"\n[p2g ratios] form {form}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(r.items())))


def reference(oracle, key, build, planes=None):
    """(scene, exact sums, the serial oracle's integer facts) of a scene, computed once per session.  planes: a function of
    the scene giving the x-planes to restrict the exact sums to (large scenes)."""
    if key not in _cache:
        n, pos, vel, solid = scene = build()
        t0 = time.time()
        ref = R.p2g_ref(pos, vel, n, solid=solid, planes=None if planes is None else planes(scene))
        t_ref = time.time() - t0
        o = oracle.Oracle(n=n)
        o.set_threads(1)
        if solid is not None:
            o.set_solid(solid)
        o.set_particles(pos, vel)
        o.p2g(); o.flags_index()
        facts = {"indices": o.field(4), "solid": o.field(9) != 0, "num_active": o.stats()["num_active"]}
        o.close()
        print(f"[{key}] n={n} particles={len(pos)} cells={len(ref.cell)} k_max={ref.k.max() if len(ref.k) else 0} "
              f"negative addends={int(ref.kneg.sum())} reference {t_ref:.2f} s")
        _cache[key] = (scene, ref, facts)
    return _cache[key]


def new_sim(fs, monkeypatch, form, n, solid=None):
    if form is None:
        monkeypatch.delenv("FLUID_P2G_FORM", raising=False)
    else:
        monkeypatch.setenv("FLUID_P2G_FORM", form)
    sim = fs.FluidSim(n=n)
    if solid is not None:
        sim.set_solid(solid)
    return sim


def device_fields(fs, sim):
    sim.p2g(); sim.flags_index()
    F = fs.FIELD
    st = sim.stats()
    return {"weights": sim.field(F.WEIGHTS), "container": sim.field(F.CONTAINER), "vel": sim.field(F.VEL),
            "vel_before": sim.field(F.VEL_BEFORE), "indices": sim.field(F.INDICES), "flags": sim.field(F.FLAGS),
            "num_active": st["num_active"], "paths": st["paths"], "box": (st["box_lo"], st["box_hi"])}


def form_ran(got):
    return "tiles" if got["paths"] & TILES else ("crowd" if got["paths"] & CROWD else "rows")


def host_choice(n, pos, got, last_active):
    """A second copy of run_p2g's choice (csrc/fluid_api.hip, `piled` / `airy` / `crowd`; P2G_PILED = 256 in csrc/common.h), to
    be kept in step with it: without it the cases that leave the choice to the host could not assert which kernel ran.
    The documented rule of the host (FLUID_PATH_P2G_CROWD: piled particles or a mostly empty box): the crowd form once a
    base cell holds more than 256 particles, or when the previous flags pass on this handle found unknowns in under 30 % of
    this call's box; else rows.  The tile form only for boxes whose partial sums would not fit (never at these sizes)."""
    lo = -(n // 2)
    b = R.c_round(pos) - lo
    on = np.all((b >= 0) & (b < n), axis=1)
    most = 0
    if on.any():
        bi = b[on].astype(np.int64)
        most = np.bincount((bi[:, 0] * n + bi[:, 1]) * n + bi[:, 2]).max()
    cells = np.prod([h - l + 1 for l, h in zip(*got["box"])])
    airy = last_active > 0 and last_active < 0.3 * cells
    return "crowd" if most > 256 or airy else "rows"


def expected_form(form, n, pos, got, last_active=0):
    """The form a call must report: the forced one, else the host's choice; a call whose particles are all off the grid has an
    empty box, launches nothing and reports no particle -> grid bit at all."""
    lo3, hi3 = got["box"]
    if any(h < l for l, h in zip(lo3, hi3)):
        return "rows"
    return form if form is not None else host_choice(n, pos, got, last_active)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def hold(label, scene, ref, facts, got, form, grazing=False, planes=None):
    """Checks 1 - 5 of the module docstring on one call's fields; form: the form this call must have taken."""
    n, pos, vel, solid = scene
    ran = form_ran(got)
    assert ran == form, (label, "asked for", form, "ran", ran, got["paths"])
    v = R.check_fields(ref, got["weights"], got["vel"], container=got["container"], solid=facts["solid"] if facts else None,
                       narrowings=NARROWINGS[ran], grazing=grazing, planes=planes)
    for what, r in v.ratio.items():
        RATIOS.setdefault(ran, {})[what] = max(RATIOS.get(ran, {}).get(what, 0.0), r)
    print(f"[{label}] form={ran} ratios={ {k: float(f'{x:.3g}') for k, x in v.ratio.items()} }")
    assert v, (label, v.describe(n))
    assert v.ambiguous == 0, label
    if not grazing:
        assert len(ref.sign_split()) == 0, label
    assert same_bits(got["vel_before"], got["vel"]), label
    assert same_bits(got["weights"], got["container"]), label       # one array on the device
    if facts is not None and not grazing:
        assert np.array_equal(got["indices"], facts["indices"]), label
        assert got["num_active"] == facts["num_active"], label
        assert np.array_equal((got["flags"] & 1) != 0, facts["solid"]), label
        assert np.array_equal((got["flags"] & 2) != 0, facts["indices"] >= 0), label
    return v


def run_case(fs, oracle, monkeypatch, key, build, form, grazing=False, planes=None):
    scene, ref, facts = reference(oracle, key, build, planes)
    n, pos, vel, solid = scene
    sim = new_sim(fs, monkeypatch, form, n, solid)
    sim.upload_particles(pos, vel)
    got = device_fields(fs, sim)
    sim.close()
    hold(f"{key}/{form}", scene, ref, facts, got, expected_form(form, n, pos, got), grazing=grazing,
         planes=None if planes is None else planes(scene))
    return scene, ref, facts, got


# ---- shapes: one, two and three z pieces, ragged last piece, odd n ---------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("n", [63, 64, 65, 96, 125, 128])
def test_full_z_extent(fs, oracle, monkeypatch, n, form):
    """Boxes (W plus its rim) of 61 .. 126 cells along z: one piece of at most 62 (n = 63, 64), two (65: 32 + 31; 96: 47 + 47;
    125: 62 + 61), three (128: 42 + 42 + 42); odd and even n."""
    run_case(fs, oracle, monkeypatch, f"tall{n}", lambda: S.tall_water(n), form)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_unit_velocity_pins_the_weight_partials(fs, oracle, monkeypatch, form):
    """v = (1, 1, 1): the numerator IS the weight sum, so the double partial sums of the weight are held to k * 2^-53."""
    _, ref, _, _ = run_case(fs, oracle, monkeypatch, "tall96_unit", lambda: S.tall_water(96, seed=5, unit_velocity=True), form)
    assert np.array_equal(ref.N[0], ref.Wp) and np.array_equal(ref.N_lo[2], ref.Wp_lo)


# ---- long rows and full plane segments, just under and just over the crowded-cell threshold ------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("ppc", [(16, 17), (18, 19)], ids=["ppc16_17", "ppc18_19"])
def test_long_rows(fs, oracle, monkeypatch, ppc, form):
    """26^3 cells of 16-17 (no cell crowded) or 18-19 particles (every cell crowded): rows of ~440 particles, more than one
    staged chunk of 384.  (Its y segments are single columns: the budget cut is test_budget_cut_*'s.)"""
    scene, ref, _, _ = run_case(fs, oracle, monkeypatch, f"dense{ppc[0]}", lambda: S.dense_rows(32, ppc), form)
    assert len(scene[1]) / 26 ** 2 > 384


def assert_segments_cut(scene, got, at_least):
    """From the call's box and the launcher's documented rule: regular y segments of two or more columns hold more than the
    work item's budget (8192 particles per z piece) and are cut further."""
    n, pos = scene[0], scene[1]
    box = got["box"]
    assert box == S.box_of(n, pos)
    ntz, zt, nseg = S.launch_cut(box)
    items = S.work_items(n, pos, box)
    cut = [(ln, c, nsub) for ln, c, nsub in items if nsub > 1]
    print(f"box {box}: ntz {ntz}, {nseg} y segments, {len(cut)} of {len(items)} (plane, segment) pairs cut further, into up to "
          f"{max(i[2] for i in items)} pieces")
    assert len(cut) >= at_least and all(ln >= 2 and c > S.P2G_BUDGET * ntz for ln, c, _ in cut)


@pytest.mark.parametrize("form", ("rows", "crowd", None), ids=str)
def test_budget_cut_around_heaps(fs, oracle, monkeypatch, form):
    """Thin water in a wide flat box with three heaps of 10 000 to 20 000 particles: the y segments around a heap exceed the
    budget and are cut, down to pieces whose rows hold the heap several times over."""
    scene, ref, facts, got = run_case(fs, oracle, monkeypatch, "heaped", S.heaped, form)
    assert_segments_cut(scene, got, 3)


def slab_planes(scene):
    """The two planes at each end of the slab's box and four seeded ones in between."""
    (x0, _, _), (x1, _, _) = S.box_of(scene[0], scene[1])
    rng = np.random.default_rng(96)
    return [x0, x0 + 1, x1 - 1, x1] + sorted(rng.choice(np.arange(x0 + 2, x1 - 1), 4, replace=False).tolist())


@pytest.mark.parametrize("form", ("rows", "crowd"), ids=str)
@pytest.mark.parametrize("ppc", [(16, 17), (18, 19)], ids=["ppc16_17", "ppc18_19"])
def test_budget_cut_in_even_water(fs, oracle, monkeypatch, ppc, form):
    """88 x 88 x 58 cells of 16-17 (no cell crowded) or 18-19 particles (every cell crowded), 7 M particles: regular y segments
    of 9 columns hold ~11 000 particles in their rows, more than the 8192 budget, with no heap anywhere, so (nearly) every
    segment of every plane is cut; rows of ~960 particles span three staged chunks.  Exact sums on 8 x-planes."""
    scene, ref, facts, got = run_case(fs, oracle, monkeypatch, f"slab{ppc[0]}", lambda: S.dense_slab(96, ppc), form, planes=slab_planes)
    assert_segments_cut(scene, got, 800)


# ---- piles and thresholds (the scenes of test_gpu_parity, now per cell) --------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_piles(fs, oracle, monkeypatch, seed, form):
    """Piles of 60 .. 12 000 particles per cell on thin water, some against the walls."""
    run_case(fs, oracle, monkeypatch, f"piles{seed}", lambda: S.piles(seed), form)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_thresholds(fs, oracle, monkeypatch, form):
    """Cells of exactly 17 / 18 / 19, 63 / 64 / 65, 511 / 512 / 513, 1024 / 1025 particles: the crowded-cell threshold, one and two
    staged batches, one, two and three pieces of a cell."""
    run_case(fs, oracle, monkeypatch, "thresholds", S.thresholds, form)


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_walls_shell_off_grid_and_obstacle(fs, oracle, monkeypatch, form):
    """Piles and single particles in the first and last cell of W on every axis, in the shell, off the grid on every side, and a
    solid slab through a pile's support."""
    scene, ref, facts, got = run_case(fs, oracle, monkeypatch, "edges", S.edges, form)
    n, pos, vel, solid = scene
    assert np.all(got["weights"][solid != 0] == 0)
    lo = -(n // 2)
    assert got["weights"][5 - lo, -5 - lo, 5 - lo] > 0 and got["weights"][6 - lo, -5 - lo, 5 - lo] == 0   # the pile and the slab


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_on_cell_centres_is_exact(fs, oracle, monkeypatch, form):
    """cw is exactly 1 or 0 and the velocities are small integers: container is the particle count and velocity the correctly
    rounded quotient, bit for bit, in every form."""
    scene, ref, _, got = run_case(fs, oracle, monkeypatch, "centres", S.on_centres, form)
    assert ref.k.max() == 3000 and np.all(ref.Wp == ref.k)
    assert np.array_equal(got["container"].reshape(-1)[ref.cell], ref.k.astype(np.float32))
    assert np.array_equal(got["vel"].reshape(3, -1)[:, ref.cell], ref.N / ref.k)


@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("which", ["empty", "one", "all_off_grid", "ties"])
def test_degenerate_sets(fs, oracle, monkeypatch, which, form):
    def build():
        n = 24
        lo, hi = S.bounds(n)
        if which == "ties":
            return S.ties(16)
        pos = {"empty": np.zeros((0, 3)), "one": np.array([[0.3, 2.2, -1.7]]),
               "all_off_grid": np.array([[hi + 2.5, 0, 0], [0, lo - 3.0, 0], [1e6, 1e6, -1e6], [0, 0, hi + 1.2]])}[which]
        return n, pos, np.full(pos.shape, 0.5), None
    scene, ref, _, got = run_case(fs, oracle, monkeypatch, which, build, form)
    assert (len(ref.cell) == 0) == (which in ("empty", "all_off_grid"))
    if len(ref.cell) == 0:
        assert got["num_active"] == 0 and not got["weights"].any() and not got["vel"].any()


# ---- grazing addends ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=str)
def test_grazing_addend_in_ordinary_water(fs, oracle, monkeypatch, form):
    """(d) a negative spline value added to a cell of ordinary water: invisible at float precision, every bar and exact fact holds."""
    scene, ref, _, _ = run_case(fs, oracle, monkeypatch, "grazing_water", lambda: S.grazing("water"), form)
    assert ref.kneg.sum() >= 3


@pytest.mark.parametrize("form", FORMS, ids=str)
@pytest.mark.parametrize("kind", S.GRAZING_KINDS)
def test_grazing_cells(fs, oracle, monkeypatch, kind, form):
    """(a)-(c) cells fed by spline noise only.  The reference adds negative addends to `weights` but not to `container`; the
    device keeps ONE array (the sum of all addends, Wp) for both.  Documented difference: the device's
    weight, its divisor and its numerators follow the exact sums as everywhere, CONTAINER is WEIGHTS, and the fluid flag is
    taken from it, so it differs from the reference's exactly in the cells where (Wc > 0) != (Wp > 0) and nowhere else."""
    scene, ref, facts = reference(oracle, f"grazing_{kind}", lambda: S.grazing(kind))
    n, pos, vel, solid = scene
    sim = new_sim(fs, monkeypatch, form, n)
    sim.upload_particles(pos, vel)
    got = device_fields(fs, sim)
    sim.close()
    hold(f"grazing_{kind}/{form}", scene, ref, facts, got, expected_form(form, n, pos, got), grazing=True)
    assert np.all((ref.Wp == 0) | (np.abs(ref.Wp) > 2.0 ** -20 * ref.A))          # no marginal sign in these scenes
    w = got["weights"].reshape(-1)
    assert np.array_equal(np.sign(w[ref.cell]), np.sign(ref.Wp))
    fluid_dev = (got["flags"].reshape(-1) & 2) != 0
    fluid_ref = facts["indices"].reshape(-1) >= 0
    assert np.array_equal(fluid_ref, ref.dense("Wc") > 0)
    differ = np.nonzero(fluid_dev != fluid_ref)[0]
    print(f"[grazing_{kind}/{form}] flag differs from the reference's in cells {differ.tolist()}; predicted {ref.flag_split().tolist()}")
    assert differ.tolist() == sorted(ref.flag_split().tolist())
    assert (len(differ) > 0) == (kind in ("pos_neg", "cancel"))
    assert got["num_active"] == np.count_nonzero(fluid_dev) == np.count_nonzero(ref.Wp > 0)
    idx = got["indices"].reshape(-1)
    assert np.array_equal(idx[fluid_dev], np.arange(np.count_nonzero(fluid_dev))) and np.all(idx[~fluid_dev] == -1)


# ---- one handle, many calls ---------------------------------------------------------------------------------------------------
REUSE_ORDER = ("big", "small_inside", "small_far", "empty", "big", "holed", "big", "wider", "small_inside", "piled", "big",
               "piled", "small_far", "holed")


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_one_handle_many_calls(fs, oracle, monkeypatch, form):
    """Every call on ONE handle is held per cell to the exact sums of that call's particles and must equal, bit for bit, a
    fresh handle given the same upload (in the form the reused handle took).  In order: a big box, a small one inside it, a
    small one far away (the sort's guess from the previous box fails: full pass), no particles, the big one again, the big
    one with the upper z piece of a bundle of columns emptied (column pieces that were written in the call before, in the same
    layout, and are flagged "not written" now: their partials of the call before must not be read), a wider box (the partial
    and work-list buffers grow inside the call), small again, piles (the host's own choice turns to the crowd form:
    parked sums, the crowded cells' list) and back."""
    n = 96
    scenes = S.reuse_scenes(n)
    sim = new_sim(fs, monkeypatch, form, n)
    last_active = 0
    taken = []
    fed = {}
    for step, name in enumerate(REUSE_ORDER):
        scene, ref, facts = reference(oracle, f"reuse_{name}", scenes[name])
        _, pos, vel, _ = scene
        sim.upload_particles(pos, vel)
        got = device_fields(fs, sim)
        hold(f"reuse[{step}] {name}/{form}", scene, ref, facts, got, expected_form(form, n, pos, got, last_active))
        taken.append(form_ran(got))
        last_active = got["num_active"]
        if name in ("big", "holed"):
            assert got["box"] == S.box_of(n, pos)
            fed[name] = (got["box"], S.fed_pieces(n, pos, got["box"]))
            if name == "holed" and REUSE_ORDER[step - 1] == "big":
                # the same box, hence the same layout of the partials, and column pieces fed in the call before and by nothing now
                assert fed["big"][0] == fed["holed"][0] and S.launch_cut(got["box"])[0] == 2
                stale = fed["big"][1] & ~fed["holed"][1]
                print(f"reuse[{step}]: {int(stale.sum())} (source plane, column, z piece) entries written in the call before, not now")
                emptied = fed["big"][1].any(axis=0) & ~fed["holed"][1].any(axis=0)    # column pieces nothing reaches any more
                assert stale.sum() >= 30 and emptied.any() and fed["holed"][1].any(axis=0).sum() > emptied.sum()
        fresh = new_sim(fs, monkeypatch, form_ran(got), n)
        fresh.upload_particles(pos, vel)
        clean = device_fields(fs, fresh)
        fresh.close()
        for f in ("weights", "vel", "vel_before", "indices", "flags"):
            assert same_bits(got[f], clean[f]), (step, name, f)
        assert got["num_active"] == clean["num_active"]
    sim.close()
    if form is None:
        pairs = set(zip(taken, taken[1:]))
        assert ("rows", "crowd") in pairs and ("crowd", "rows") in pairs, taken   # each followed the other on the one handle
        print("forms taken by the host:", taken)


def test_upload_order_does_not_reach_the_sums(fs, oracle, monkeypatch):
    """The same particles with the same ids in two upload orders: the fields are equal bit for bit (the sum order is a pure
    function of the input: rows, source cells, then ids)."""
    scene, ref, facts = reference(oracle, "piles2", lambda: S.piles(2))
    n, pos, vel, _ = scene
    ids = np.arange(len(pos), dtype=np.uint32)
    rng = np.random.default_rng(3)
    out = {}
    for form in ("rows", "crowd", "tiles"):
        for order in ("given", "shuffled", "reversed"):
            o = {"given": np.arange(len(pos)), "shuffled": rng.permutation(len(pos)), "reversed": np.arange(len(pos))[::-1]}[order]
            sim = new_sim(fs, monkeypatch, form, n)
            sim.upload_particles_ids(pos[o], vel[o], ids[o])
            got = device_fields(fs, sim)
            sim.close()
            hold(f"ids {order}/{form}", scene, ref, facts, got, form)
            if form in out:
                for f in ("weights", "vel", "indices", "flags"):
                    assert same_bits(got[f], out[form][f]), (form, order, f)
            out[form] = got
        # and the ids given by upload_particles (0 .. n-1 in upload order) are the same thing
        sim = new_sim(fs, monkeypatch, form, n)
        sim.upload_particles(pos, vel)
        got = device_fields(fs, sim)
        sim.close()
        assert same_bits(got["weights"], out[form]["weights"]) and same_bits(got["vel"], out[form]["vel"])


@pytest.mark.parametrize("form", [None, "crowd"], ids=str)
def test_after_whole_steps(fs, oracle, monkeypatch, form):
    """Two whole steps, then a fresh upload and p2g() on the same handle: the step's state (boxes, dirty fields, sort hint,
    the handle's last unknown count) does not reach the sums."""
    n = 64
    scene, ref, facts = reference(oracle, "tall64", lambda: S.tall_water(64))
    _, pos, vel, _ = scene
    sim = new_sim(fs, monkeypatch, form, n)
    _, first, _, _ = S.water(n, 6, seed=11)
    sim.upload_particles(first)
    last = 0
    for _ in range(2):
        last = sim.step()["num_active"]
    sim.upload_particles(pos, vel)
    got = device_fields(fs, sim)
    sim.close()
    hold(f"after steps/{form}", scene, ref, facts, got, expected_form(form, n, pos, got, last))
    fresh = new_sim(fs, monkeypatch, form_ran(got), n)
    fresh.upload_particles(pos, vel)
    clean = device_fields(fs, fresh)
    fresh.close()
    for f in ("weights", "vel", "vel_before", "indices", "flags"):
        assert same_bits(got[f], clean[f]), f


# ---- the bench scene ---------------------------------------------------------------------------------------------------------
def test_bench_scene_planes_at_256(fs, oracle, monkeypatch):
    """water_cube_drop(256, 8), 5.3 M particles, the host's own form: whole x-planes against the exact sums.  The launcher cuts
    y into segments and z into pieces inside every x-plane, so each checked plane holds every y-segment and z-piece boundary of
    this scene (z: 89 cells = 45 + 44); the planes are the two at each end of the box (the box's rim, which receives only
    from its inner neighbour, and the first plane holding particles) and 8 seeded ones in between."""
    n = 256
    pos = fs.water_cube_drop(n, 8, seed=0)
    rng = np.random.default_rng(256)
    vel = rng.standard_normal(pos.shape)
    sim = new_sim(fs, monkeypatch, None, n)
    sim.upload_particles(pos, vel)
    got = device_fields(fs, sim)
    sim.close()
    (x0, y0, z0), (x1, y1, z1) = got["box"]
    assert z1 - z0 + 1 > 62 and x1 - x0 + 1 > 80
    planes = [x0, x0 + 1, x1 - 1, x1] + sorted(rng.choice(np.arange(x0 + 2, x1 - 1), 8, replace=False).tolist())
    t0 = time.time()
    ref = R.p2g_ref(pos, vel, n, planes=planes)
    t_ref = time.time() - t0
    print(f"[bench256] box x {x0}..{x1} y {y0}..{y1} z {z0}..{z1}; planes {planes}; cells {len(ref.cell)}; k_max {ref.k.max()}; "
          f"negative addends {int(ref.kneg.sum())}; reference {t_ref:.1f} s")
    assert set(np.unique(ref.cell // (n * n)).tolist()) == set(planes)
    o = oracle.Oracle(n=n)
    o.set_threads(1)
    o.set_particles(pos, vel)
    o.p2g(); o.flags_index()
    facts = {"indices": o.field(4), "solid": o.field(9) != 0, "num_active": o.stats()["num_active"]}
    o.close()
    hold("bench256", (n, pos, vel, None), ref, facts, got, expected_form(None, n, pos, got), planes=planes)
    # outside the box every field is exactly 0, on the whole grid
    inside = np.zeros((n, n, n), dtype=bool)
    inside[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = True
    assert not got["weights"][~inside].any() and not got["vel"][:, ~inside].any()
