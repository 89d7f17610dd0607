"""The numpy V-cycles of tests/mg_ref.py checked by themselves, before any kernel is held to them (CPU only).

M^-1 of either cycle is a fixed linear operator that the design makes symmetric positive definite: reversed sweep weights after the
correction, restriction = transposed prolongation up to a scalar, a scalar weight on every correction, a symmetric coarsest solve.
So symmetry, definiteness and linearity hold to rounding, the Galerkin rows equal a dense triple product exactly, the cycle must be
worth having (PCG iteration counts), and the four classic mistakes each move z by orders of magnitude more than the bars that
tests/test_gpu_vcycle.py allows the kernels.
"""
import numpy as np
import pytest

import mg_ref
import pressure_system as ps

DT = 0.1    # scale = dt / (rho dx^2): not a power of two, so the float-accumulated diagonal table differs from k x scale

# the scenes of tests/test_gpu_vcycle.py at reduced size (odd and even level sizes among them)
SMALL = [("tank", 12), ("tank", 13), ("holes", 16), ("pool", 20), ("floor", 16), ("floor_odd", 17)]


def domain(name, n):
    """Level-0 types and counts of a scene whose active box is the whole grid."""
    solid, cont = mg_ref.scene(name, n)
    typ, cnt = mg_ref.level0_types(solid, cont > 0, (0, 0, 0), (n - 1, n - 1, n - 1))
    return solid, cont, typ, cnt


def cycles(name, n, T=np.float64, **kw):
    _, _, typ, cnt = domain(name, n)
    return typ, {"mg": mg_ref.Rediscretised(typ, cnt, DT, T), "gal": mg_ref.Galerkin(typ, cnt, DT, T, lc=2)}


def rand_rhs(typ, seed):
    rng = np.random.default_rng(seed)
    return np.where(typ == 2, rng.uniform(-1, 1, typ.shape), 0).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("name,n", SMALL)
def test_symmetry(name, n):
    typ, cyc = cycles(name, n)
    assert (typ == 2).sum() > 20
    a, b = rand_rhs(typ, 1), rand_rhs(typ, 2)
    for key, M in cyc.items():
        za, zb = M(a), M(b)
        lhs, rhs = np.sum(za * b), np.sum(a * zb)
        rel = abs(lhs - rhs) / (np.linalg.norm(za) * np.linalg.norm(b))
        print(f"{name} {n} {key}: <M^-1 a, b> = {lhs:.17g}, <a, M^-1 b> = {rhs:.17g}, rel {rel:.2e}")
        assert rel <= 1e-12, (key, rel)
        assert not za[typ != 2].any()


def test_positive_definite():
    typ, cyc = cycles("holes", 10)
    unknowns = np.argwhere(typ == 2)
    assert len(unknowns) > 100
    for key, M in cyc.items():
        for seed in range(20):
            b = rand_rhs(typ, 100 + seed)
            assert np.sum(b * M(b)) > 0, (key, seed)
        for c in unknowns:
            b = np.zeros(typ.shape)
            b[tuple(c)] = 1.0
            assert M(b)[tuple(c)] > 0, (key, tuple(c))


@pytest.mark.parametrize("name,n", [("holes", 16), ("pool", 20)])
def test_linearity(name, n):
    typ, cyc = cycles(name, n)
    a, b = rand_rhs(typ, 3), rand_rhs(typ, 4)
    for key, M in cyc.items():
        lhs, rhs = M(a + 2 * b), M(a) + 2 * M(b)
        assert np.abs(lhs - rhs).max() <= 1e-13 * np.abs(rhs).max(), key


def test_level0_rows_are_the_pressure_system():
    """The level-0 operator of the reference against tests/pressure_system.py, entry by entry."""
    n = 12
    solid, cont, typ, cnt = domain("holes", n)
    fluid = (cont > 0) & (solid == 0)
    idx = np.full(n ** 3, -1, dtype=np.int32)
    idx[np.flatnonzero(fluid)] = np.arange(fluid.sum())
    sys = ps.restate(solid, cont, idx, DT)
    rows, cols, vals = sys.triplets()
    want = np.zeros((sys.size, sys.size))
    want[rows, cols] = vals
    A, cells = mg_ref.op_level0(typ, cnt, DT, np.float64).dense()
    # level-0 cell (i, j, k) is grid cell (i - 1, j - 1, k - 1)
    i, j, k = np.unravel_index(cells, typ.shape)
    grid = ((i - 1) * n + (j - 1)) * n + (k - 1)
    keep = sys.in_system
    assert np.array_equal(grid, sys.cells[keep])
    assert np.array_equal(A, want[np.ix_(keep, keep)])


def test_galerkin_rows_are_the_triple_product():
    """gd, gx, gy, gz of levels 1 and 2 expanded to dense matrices equal P^T A P formed densely from the level below: exactly, in
    float64 (every entry is a small integer times a float32 number)."""
    _, _, typ, cnt = domain("holes", 12)
    gal = mg_ref.Galerkin(typ, cnt, DT, np.float64, lc=2)
    assert (typ == 1).any() and (typ == 0)[2:-2, 2:-2, 2:-2].any()
    for l in (1, 2):
        fine, coarse = gal.ops[l - 1], gal.ops[l]
        Af, fcells = fine.dense()
        Ac, ccells = coarse.dense()
        i, j, k = np.unravel_index(fcells, fine.mask.shape)
        parent = np.ravel_multi_index((i >> 1, j >> 1, k >> 1), coarse.mask.shape)
        assert np.array_equal(np.unique(parent), ccells)
        P = (parent[:, None] == ccells[None, :]).astype(np.float64)
        assert len(ccells) > 8 and np.array_equal(P.T @ Af @ P, Ac), l


def _pcg(op, b, minv, tol=1e-10, cap=2000):
    x = np.zeros_like(b)
    r = b.copy()
    z = minv(r)
    s = z.copy()
    rz = np.sum(r * z)
    nb = np.linalg.norm(b)
    for it in range(1, cap + 1):
        q = op.apply(s)
        alpha = rz / np.sum(s * q)
        x += alpha * s
        r -= alpha * q
        if np.linalg.norm(r) <= tol * nb:
            return it
        z = minv(r)
        rz, old = np.sum(r * z), rz
        s = z + (rz / old) * s
    return cap + 1


@pytest.mark.parametrize("name", ["tank", "pool"])
def test_cycle_is_worth_having(name):
    """PCG to 1e-10 on a 32^3 full tank and a 32^3 shallow pool: a cycle that is symmetric but does nothing would pass the tests above.
    The re-discretised cycle may need at most 1.25 x (Jacobi-preconditioned CG's count / 5).  Counts (Jacobi / re-discretised /
    Galerkin): tank 257 / 23 / 24, pool 79 / 12 / 12."""
    n = 32
    typ, cyc = cycles(name, n)
    op = cyc["mg"].ops[0]
    b = rand_rhs(typ, 7)
    jac = _pcg(op, b, lambda r: op.inv * r)
    mg = _pcg(op, b, cyc["mg"])
    gal = _pcg(op, b, cyc["gal"])
    print(f"{name} {n}^3: Jacobi {jac}, re-discretised {mg}, Galerkin {gal} iterations")
    assert mg <= 1.25 * jac / 5, (jac, mg)
    assert gal < jac


def test_mutations_clear_the_bars():
    """Scene A of tests/test_gpu_vcycle.py (24^3 full tank).  Each classic mistake moves z by more than 100 x the fp32 bar
    (4 x the difference between the float32 and the float64 run of the reference), so the bar separates right from wrong.

    One mistake on the list this test was written from cannot be seen by any test, here or on the GPU: the two sweeps after the
    correction in (W1, W2) instead of (W2, W1) order.  A damped-Jacobi sweep is the affine map v -> v + w D^-1 (f - A v); two of
    them with weights w1, w2 apply the polynomial (1 - w1 x)(1 - w2 x) of x = D^-1 A to the error, whichever comes first, so the
    order changes z by rounding only and M stays symmetric.  The test asserts exactly that (the move is 3.5e-16 of max|z|), so
    nobody has to find it out again; what the reversal is there to guard — a symmetric M — is covered by the coarsest level's
    colour order below and by the symmetry tests."""
    _, _, typ, cnt = domain("tank", 24)
    b = rand_rhs(typ, 5)

    def dist(z, ref):
        return np.abs(z.astype(np.float64) - ref).max() / np.abs(ref).max()

    mg64 = mg_ref.Rediscretised(typ, cnt, DT, np.float64, elem=4)(b)
    gal64 = mg_ref.Galerkin(typ, cnt, DT, np.float64)(b)
    bar_mg = 4 * dist(mg_ref.Rediscretised(typ, cnt, DT, np.float32)(b), mg64)
    bar_gal = 4 * dist(mg_ref.Galerkin(typ, cnt, DT, np.float32)(b), gal64)
    print(f"fp32 bars: re-discretised {bar_mg:.2e}, Galerkin {bar_gal:.2e}")
    assert 0 < bar_mg < 1e-5 and 0 < bar_gal < 1e-5
    wc = mg_ref.plan(typ.shape, 4)["wc"]
    mutants = {
        "coarsest colours in the same order both ways": (mg_ref.Rediscretised(typ, cnt, DT, np.float64, elem=4, coarse_colours=((0, 1), (0, 1)))(b), mg64, bar_mg),
        "3/4 <-> 1/4": (mg_ref.Rediscretised(typ, cnt, DT, np.float64, elem=4, near=0.25, far=0.75)(b), mg64, bar_mg),
        "wc[0] = 1": (mg_ref.Rediscretised(typ, cnt, DT, np.float64, elem=4, wc=[1.0] + wc[1:])(b), mg64, bar_mg),
        "Galerkin inner once": (mg_ref.Galerkin(typ, cnt, DT, np.float64, inner_factor=1)(b), gal64, bar_gal),
    }
    swapped = dist(mg_ref.Rediscretised(typ, cnt, DT, np.float64, elem=4, post=(mg_ref.MG_W1, mg_ref.MG_W2))(b), mg64)
    print(f"W1 and W2 swapped after the correction: moves z by {swapped:.2e} (two Jacobi sweeps commute)")
    assert swapped <= 1e-13
    for name, (z, ref, bar) in mutants.items():
        d = dist(z, ref)
        print(f"{name}: moves z by {d:.2e} = {d / bar:.0f} x the bar")
        assert d > 100 * bar, name


def test_plans():
    """mg_setup's decisions for the scenes of tests/test_gpu_vcycle.py (its docstring states them)."""
    p = mg_ref.plan((26, 26, 26), 4)
    assert p["dims"] == [(26,) * 3, (13,) * 3, (7,) * 3] and p["tail"] == 1 and p["fold"] and p["wc"] == [1.25, 1.0]
    assert mg_ref.plan((26, 26, 26), 8)["tail"] == 1
    for elem in (4, 8):
        p = mg_ref.plan((66, 66, 66), elem)
        assert [d[0] for d in p["dims"]] == [66, 33, 17, 9, 5] and p["tail"] == 3 and not p["fold"] and p["wc"] == [1.25, 1.1, 1.0, 1.0]
    assert mg_ref.plan((66, 66, 66), 4)["gal_lc"] == 3
    p = mg_ref.plan((106, 106, 106), 4)
    assert [d[0] for d in p["dims"]] == [106, 53, 27, 14, 7] and p["tail"] == 3
    # the smallest full-grid box whose level 2 is too large for the tail (17^3 > 4096 cells): n = 63
    assert mg_ref.plan((64, 64, 64), 4)["tail"] == 2 and mg_ref.plan((65, 65, 65), 4)["tail"] == 3


def test_stored_galerkin_rows_stay_close_and_symmetric():
    """The rows as the solver stores them (float32, children summed in index order) against the exact triple product: the same
    unknowns, every entry within 2e-6 of the level's largest diagonal, and a cycle that is still symmetric — the rounding sits in
    the diagonal and in face weights that both sides of a face share."""
    _, _, typ, cnt = domain("pool", 20)
    exact = mg_ref.Galerkin(typ, cnt, DT, np.float64, lc=2)
    stored = mg_ref.Galerkin(typ, cnt, DT, np.float64, lc=2, stored_rows=True)
    for l in (1, 2):
        e, s = exact.ops[l], stored.ops[l]
        assert np.array_equal(e.mask, s.mask)
        for name in ("gd", "wx", "wy", "wz"):
            assert np.abs(getattr(e, name) - getattr(s, name)).max() <= 2e-6 * e.gd.max(), (l, name)
    a, b = rand_rhs(typ, 1), rand_rhs(typ, 2)
    za, zb = stored(a), stored(b)
    assert abs(np.sum(za * b) - np.sum(a * zb)) <= 1e-12 * np.linalg.norm(za) * np.linalg.norm(b)
    assert np.abs(za - exact(a)).max() <= 1e-4 * np.abs(za).max()
