"""CPU: pin tests/p2g_ref.py (the exact per-cell sums of particle -> grid) and the bars derived from the reference's arithmetic.

(a) the exact sums equal a plain-Python Fraction evaluation, correctly rounded to double, in every cell of small scenes;
(b) the serial oracle lies inside the reference bars in every cell of every scene family the GPU tests use (at n <= 64);
(c) the check discriminates: a mutated restatement (one particle less or twice, another rounding rule, a wider W, a solid
    cell taken for open) fails in the cell the mutation touches, and another association of the product still passes.
"""
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import p2g_ref as R
import p2g_scenes as S


# ---- (a) the reference against Fractions -----------------------------------------------------------------------------------
def py_spline(x):
    """fluid.cc:22-37 on one Python float."""
    if x < 0:
        x *= -1.0
    if x < 0.5:
        return 1.5 * (4.0 * x * x * x - 4.0 * x * x + 2.0 / 3.0)
    if x < 1.0:
        return 1.5 * ((-8.0 * (x * x * x) / 6.0) + 4.0 * x * x - 4.0 * x + 4.0 / 3.0)
    return 0.0


def py_round(x):
    """C round(): half away from zero."""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def fraction_sums(n, pos, vel, solid):
    """cell -> [k, Wp, Wc, Nx, Ny, Nz] with exact rationals; a loop over particles and their 27 cells, as the reference's."""
    glo = -(n // 2)
    out = {}
    for p, v in zip(pos.tolist(), vel.tolist()):
        if not all(abs(c) < 1e9 for c in p):
            continue
        f = [py_round(c) for c in p]
        for x in range(f[0] - 1, f[0] + 2):
            for y in range(f[1] - 1, f[1] + 2):
                for z in range(f[2] - 1, f[2] + 2):
                    i = (x - glo, y - glo, z - glo)
                    if not all(2 <= c <= n - 3 for c in i):
                        continue
                    if solid is not None and solid[i]:
                        continue
                    cw = py_spline(p[0] - x) * py_spline(p[1] - y) * py_spline(p[2] - z)
                    if cw == 0:
                        continue
                    e = out.setdefault((i[0] * n + i[1]) * n + i[2], [0, Fraction(0), Fraction(0)] + [Fraction(0)] * 3)
                    fc = Fraction(cw)
                    e[0] += 1
                    e[1] += fc
                    if cw > 0:
                        e[2] += fc
                    for a in range(3):
                        e[3 + a] += fc * Fraction(v[a])
    return out


def small_scenes():
    rng = np.random.default_rng(42)
    n = 16
    lo, hi = S.bounds(n)
    yield "random water", n, rng.uniform(-3, 3, size=(600, 3)), None
    yield "pile of 2000", n, np.array([1.0, -2.0, 2.0]) + rng.uniform(-0.49, 0.49, size=(2000, 3)), None
    yield "ties", S.ties(16)[0], S.ties(16)[1], None
    shell = np.concatenate([rng.uniform(lo - 0.4, lo + 2.4, size=(150, 3)), rng.uniform(hi - 2.4, hi + 0.4, size=(150, 3))])
    yield "shell", n, shell, None
    off = np.concatenate([rng.uniform(lo - 3, lo + 1, size=(100, 3)), rng.uniform(hi - 1, hi + 3, size=(100, 3)), [[1e7, 0, 0], [0, -1e12, 0]]])
    yield "off grid", n, off, None
    _, pos, _, solid = S.edges(16, pile=60)
    yield "obstacle", 16, pos, solid
    _, pos, _, _ = S.grazing("pos_neg", 16)
    yield "grazing", 16, pos, None


@pytest.mark.parametrize("name,n,pos,solid", list(small_scenes()), ids=[s[0].replace(" ", "_") for s in small_scenes()])
def test_exact_sums_equal_fractions(name, n, pos, solid):
    rng = np.random.default_rng(7)
    vel = rng.standard_normal(pos.shape) * 3
    ref = R.p2g_ref(pos, vel, n, solid=solid, chunk=257)   # several chunks: the merge is part of what is pinned
    fr = fraction_sums(n, pos, vel, solid)
    assert sorted(fr) == ref.cell.tolist()
    for j, c in enumerate(ref.cell.tolist()):
        k, wp, wc, *nn = fr[c]
        assert ref.k[j] == k, (name, c)
        assert ref.Wp[j] == float(wp) and ref.Wc[j] == float(wc), (name, c)
        for a in range(3):
            assert ref.N[a][j] == float(nn[a]), (name, c, a)
            # the pair is far more exact than the double alone
            got = Fraction(float(ref.N[a][j])) + Fraction(float(ref.N_lo[a][j]))
            assert abs(got - nn[a]) <= Fraction(float(ref.T[a][j])) / 2 ** 90, (name, c, a)
    if name == "pile of 2000":
        assert ref.k.max() == 2000


# ---- (b) the serial oracle inside the reference bars -----------------------------------------------------------------------
def oracle_fields(oracle, n, pos, vel, solid):
    o = oracle.Oracle(n=n)
    o.set_threads(1)
    if solid is not None:
        o.set_solid(solid)
    o.set_particles(pos, vel)
    o.p2g(); o.flags_index()
    out = {"weights": o.field(1), "container": o.field(0), "vel": o.field(2), "indices": o.field(4), "num_active": o.stats()["num_active"]}
    o.close()
    return out


@pytest.mark.parametrize("family", sorted(S.cpu_families()))
def test_serial_oracle_is_inside_the_reference_bars(oracle, family):
    n, pos, vel, solid = S.cpu_families()[family]()
    t0 = time.time()
    ref = R.p2g_ref(pos, vel, n, solid=solid)
    t_ref = time.time() - t0
    f = oracle_fields(oracle, n, pos, vel, solid)
    v = R.check_fields(ref, f["weights"], f["vel"], container=f["container"], solid=solid if solid is not None else S.shell(n))
    print(f"{family}: n={n} particles={len(pos)} cells={len(ref.cell)} k_max={ref.k.max() if len(ref.k) else 0} negative addends={ref.kneg.sum()} "
          f"ratios={ {k: round(x, 3) for k, x in v.ratio.items()} } reference {t_ref:.2f} s")
    assert v, v.describe(n)
    assert v.ambiguous == 0
    assert len(ref.sign_split()) == 0
    assert np.array_equal(f["indices"].reshape(-1) >= 0, ref.dense("Wc") > 0)


def test_scenes_reach_the_launchers_cuts():
    """The scenes built to reach a path of the row form's work decomposition do reach it, by the launcher's documented rule
    (restated in p2g_scenes): the holed reuse scene empties column pieces that the big one fed, in the same box and two z
    pieces; the heaped scene has y segments of several columns over the 8192-particle budget."""
    sc = S.reuse_scenes(96)
    n, big, _, _ = sc["big"]()
    _, holed, _, _ = sc["holed"]()
    box = S.box_of(n, big)
    assert box == S.box_of(n, holed) and S.launch_cut(box)[:2] == (2, 47)
    fb, fh = S.fed_pieces(n, big, box), S.fed_pieces(n, holed, box)
    assert not (fh & ~fb).any() and (fb & ~fh).sum() >= 30 and (fb.any(axis=0) & ~fh.any(axis=0)).any()
    n, pos, _, _ = S.heaped()
    box = S.box_of(n, pos)
    ntz = S.launch_cut(box)[0]
    cut = [i for i in S.work_items(n, pos, box) if i[2] > 1]
    assert len(cut) >= 3 and all(ln >= 2 and c > S.P2G_BUDGET * ntz for ln, c, _ in cut)


def test_on_centres_is_exact(oracle):
    """cw is 1 or 0: container is the particle count and velocity the correctly rounded integer quotient."""
    n, pos, vel, solid = S.on_centres(24)
    ref = R.p2g_ref(pos, vel, n)
    assert np.all(ref.Wp == ref.k) and np.all(ref.Wp_lo == 0) and np.all(ref.N_lo == 0) and ref.k.max() == 3000
    f = oracle_fields(oracle, n, pos, vel, solid)
    assert np.array_equal(f["weights"].reshape(-1)[ref.cell], ref.k.astype(np.float32))
    assert np.array_equal(f["vel"].reshape(3, -1)[:, ref.cell], ref.N / ref.k)


@pytest.mark.parametrize("kind", S.GRAZING_KINDS)
def test_grazing_cells_in_the_reference(oracle, kind):
    """Cells fed by spline noise: the reference's weights follow Wp (negative addends included), its container follows Wc
    (positive addends only), the fluid flag is container > 0 and the divisor is weights."""
    n, pos, vel, solid = S.grazing(kind)
    ref = R.p2g_ref(pos, vel, n)
    f = oracle_fields(oracle, n, pos, vel, solid)
    v = R.check_fields(ref, f["weights"], f["vel"], grazing=True)
    assert v, v.describe(n)
    expect = {"neg_only": (-1, 0), "pos_neg": (-1, 1), "neg_pos": (1, 1), "cancel": (0, 1)}[kind]
    for t in S.grazing_targets(n):
        j = np.searchsorted(ref.cell, cell_of(n, t))
        assert ref.cell[j] == cell_of(n, t) and ref.kneg[j] == 1
        assert (np.sign(ref.Wp[j]), np.sign(ref.Wc[j])) == expect, (kind, t)
        assert (cell_of(n, t) in ref.sign_split()) == (expect[0] != expect[1])
    c = f["container"].reshape(-1)
    w = f["weights"].reshape(-1)
    kpos = ref.k - ref.kneg
    assert np.all(np.abs(c[ref.cell].astype(np.float64) - ref.Wc) <= R.gamma(kpos, R.U24) * ref.Wc)
    assert np.array_equal(f["indices"].reshape(-1) >= 0, ref.dense("Wc") > 0)
    assert f["num_active"] == np.count_nonzero(ref.Wc > 0)
    # no marginal sign in these scenes: Wp is exactly 0 or well clear of the float32 rounding of its addends
    assert np.all((ref.Wp == 0) | (np.abs(ref.Wp) > 2.0 ** -20 * ref.A))
    assert np.array_equal(np.sign(w[ref.cell]), np.sign(ref.Wp))
    # where a flag taken from the weights would differ from the reference's (container > 0): the targets of two of the kinds
    want = [cell_of(n, t) for t in S.grazing_targets(n)] if kind in ("pos_neg", "cancel") else []
    assert sorted(ref.flag_split().tolist()) == sorted(want)


# ---- (c) the check discriminates -------------------------------------------------------------------------------------------
def cell_of(n, coord):
    lo = -(n // 2)
    i = [int(c) - lo for c in coord]
    return (i[0] * n + i[1]) * n + i[2]


@pytest.fixture(scope="module")
def pile_scene(oracle):
    """A 12 000-particle cell and an 8-particle cell on thin water, and the serial oracle's fields for it."""
    n = 24
    rng = np.random.default_rng(5)
    big, small = np.array([3.0, -2.0, 4.0]), np.array([-6.0, 5.0, -5.0])
    pos = np.concatenate([big + rng.uniform(-0.49, 0.49, size=(12000, 3)), small + rng.uniform(-0.49, 0.49, size=(8, 3)),
                          S.water(n, 2, seed=6)[1]])
    vel = rng.standard_normal(pos.shape)
    return n, pos, vel, cell_of(n, big), cell_of(n, small), oracle_fields(oracle, n, pos, vel, None)


def test_unmutated_passes(pile_scene):
    n, pos, vel, cb, cs, f = pile_scene
    v = R.check_fields(R.p2g_ref(pos, vel, n), f["weights"], f["vel"], container=f["container"])
    assert v, v.describe(n)


@pytest.mark.parametrize("which", ["big", "small"])
def test_one_particle_removed_fails_in_its_cell(pile_scene, which):
    n, pos, vel, cb, cs, f = pile_scene
    drop, cell = (11999, cb) if which == "big" else (12007, cs)
    keep = np.arange(len(pos)) != drop
    v = R.check_fields(R.p2g_ref(pos[keep], vel[keep], n), f["weights"], f["vel"])
    assert cell in v.cells("numerator"), v.describe(n)


def test_one_particle_twice_fails_in_its_cell(pile_scene):
    n, pos, vel, cb, cs, f = pile_scene
    twice = np.concatenate([np.arange(len(pos)), [5]])
    v = R.check_fields(R.p2g_ref(pos[twice], vel[twice], n), f["weights"], f["vel"])
    assert cb in v.cells("numerator"), v.describe(n)


def test_floor_rounding_on_a_negative_tie_cannot_show_in_the_sums(oracle):
    """floor(x + 0.5) instead of C round moves the base cell of a particle at a negative x.5 (-2.5: -2 instead of -3).  That is
    the only place the two rules differ, and there the cell the one rule reaches and the other does not lies at distance
    exactly 1.5, where spline() is 0: the addend is dropped (cw == 0) under either rule.  So this mutation has no cell to fail
    in: the exact sums are identical, in the interior and against the wall, and the test pins that instead (the base cell itself
    is pinned where it matters, in the sort's histogram: tests/sources_ref.base_cell_counts)."""
    n = 16
    lo = -(n // 2)
    floor_rule = lambda x: np.floor(x + 0.5)
    pos = np.array([[-2.5, 0.25, 0.25], [-2.5, -1.5, -0.5], [lo + 1.5, 0.25, 0.25], [lo + 2.5, lo + 2.5, 0.1], [1.3, 1.2, -0.7], [2.5, 0.1, 0.2]])
    vel = np.arange(18, dtype=np.float64).reshape(6, 3) - 7
    assert not np.array_equal(R.c_round(pos), floor_rule(pos))
    good, bad = R.p2g_ref(pos, vel, n), R.p2g_ref(pos, vel, n, round_fn=floor_rule)
    assert good.cell.tolist() == bad.cell.tolist() and np.array_equal(good.k, bad.k)
    assert np.array_equal(good.Wp, bad.Wp) and np.array_equal(good.N, bad.N) and np.array_equal(good.N_lo, bad.N_lo)
    f = oracle_fields(oracle, n, pos, vel, None)
    v = R.check_fields(good, f["weights"], f["vel"], container=f["container"])
    assert v, v.describe(n)


def test_wider_w_fails_in_the_shell(oracle):
    n = 16
    lo = -(n // 2)
    pos = np.array([[lo + 1.8, 0.3, 0.1], [0.2, 0.3, 0.4]])
    vel = np.ones_like(pos)
    f = oracle_fields(oracle, n, pos, vel, None)
    assert R.check_fields(R.p2g_ref(pos, vel, n), f["weights"], f["vel"])
    v = R.check_fields(R.p2g_ref(pos, vel, n, w_margin=1), f["weights"], f["vel"])
    assert cell_of(n, (lo + 1, 0, 0)) in v.cells("support"), v.describe(n)


def test_solid_taken_for_open_fails_in_the_solid_cell(oracle):
    n, pos, vel, solid = S.edges(24)
    f = oracle_fields(oracle, n, pos, vel, solid)
    assert R.check_fields(R.p2g_ref(pos, vel, n, solid=solid), f["weights"], f["vel"], solid=solid)
    v = R.check_fields(R.p2g_ref(pos, vel, n, solid=None), f["weights"], f["vel"])
    assert cell_of(n, (5, -5, 6)) in v.cells("support"), v.describe(n)


def test_other_association_still_passes(pile_scene):
    """sx * (sy * sz): two more roundings per addend, inside gamma(k + 4).  The bar pins sums, not an association."""
    n, pos, vel, cb, cs, f = pile_scene
    ref = R.p2g_ref(pos, vel, n, assoc="x_yz")
    assert not np.array_equal(ref.Wp, R.p2g_ref(pos, vel, n).Wp)
    v = R.check_fields(ref, f["weights"], f["vel"])
    assert v, v.describe(n)
