"""CPU (-m "not gpu"): pins tests/pressure_system.py, the true-residual check of every pressure solve.

 * the restated matrix is oracle.system()'s, entry for entry, on the awkward shapes, an obstacle and a pool that has settled;
 * residual() agrees with an exact rational evaluation to the last bit;
 * calibration: the oracle's Jacobi CG and the vendored Eigen IC-PCG (when oracle/_ref is built) sit >= 4x under the bars;
 * sensitivity: a 1e-14 relative perturbation of p fails the eta bar, a 1e-13 change of one cell fails the omega bar.
"""
import decimal
from fractions import Fraction

import numpy as np
import pytest

import pressure_system as ps
from test_gpu_parity import _shape_particles

SHAPES = ["sheet", "needle", "blobs", "corner", "odd"]


def _solved(oracle, o):
    """One pass's system as the oracle solves it: rhs, matrix, solve, then the triplets with the b that solve used
    (oracle.system() re-reads b from DIVER, which a whole pressure_pass() has already overwritten with b2)."""
    o.rhs_div(); o.build_matrix(); o.solve()
    rows, cols, vals, b, _, p = o.system()
    sys_ = ps.restate(o.field(9), o.field(0), o.field(4), o.dt)
    sys_.solid = o.field(9)
    return sys_, (rows, cols, vals), b, p


def _scene(fs, oracle, name):
    if name in SHAPES:
        n = 48
        o = oracle.Oracle(n=n)
        pos = _shape_particles(fs, n, name, np.random.default_rng(5))
        o.set_particles(pos, np.random.default_rng(6).standard_normal(pos.shape))   # a right-hand side in every cell
        o.p2g(); o.flags_index()
        return o
    if name == "obstacle":        # a solid block inside the falling cube and a post on the floor
        n = 32
        pos = fs.water_cube_drop(n, 4, seed=3)
        solid = np.zeros((n, n, n), dtype=np.uint8)
        solid[:2], solid[-2:], solid[:, :2], solid[:, -2:], solid[:, :, :2], solid[:, :, -2:] = 1, 1, 1, 1, 1, 1
        c = np.round(pos.mean(0)).astype(int) - fs.grid_bounds(n)[0]
        solid[c[0] - 2:c[0] + 2, c[1] - 1:c[1] + 3, c[2] - 3:c[2] + 1] = 1
        solid[4:8, 2:10, 20:23] = 1
        o = oracle.Oracle(n=n)
        o.set_solid(solid)
        o.set_particles(pos, np.random.default_rng(6).standard_normal(pos.shape))
        o.p2g(); o.flags_index()
        return o
    if name == "pool30":           # 40^3 after 30 steps: the cube has hit the floor and spreads
        n = 40
        o = oracle.Oracle(n=n)
        o.set_particles(fs.water_cube_drop(n, 4, seed=0))
        for _ in range(30):
            o.step()
        o.p2g(); o.flags_index()
        return o
    raise ValueError(name)


SCENES = SHAPES + ["obstacle", "pool30"]


@pytest.fixture(scope="module")
def systems(fs, oracle):
    out = {}
    for name in SCENES:
        o = _scene(fs, oracle, name)
        out[name] = _solved(oracle, o)
        o.close()
    return out


@pytest.mark.parametrize("name", SCENES)
def test_restated_matrix_is_the_oracles(systems, name):
    sys_, (rows, cols, vals), b, _ = systems[name]
    r, c, v = sys_.triplets()
    o = np.lexsort((cols, rows))
    assert len(r) == len(rows) and len(b) == sys_.size
    assert np.array_equal(r, rows[o]) and np.array_equal(c, cols[o])
    assert np.array_equal(v, vals[o])                           # bit for bit: float32 diagonal table, float32(-scale)
    assert sys_.in_system.all() or name in SHAPES               # walled-in single cells only where a shape makes them
    assert set(np.unique(sys_.count)) <= set(range(1, 7))


def test_restated_counts_are_the_flags_count_bits(systems):
    """check_field_solve's consistency check on a FLAGS array built the way flags_index builds it (bit 1 fluid, bits 2-4 count)."""
    sys_, _, b, p = systems["obstacle"]
    n = sys_.n
    flags = np.zeros(n ** 3, dtype=np.uint8)
    flags[sys_.cells] = (2 | (sys_.count << 2)).astype(np.uint8)
    idx = np.full(n ** 3, -1, dtype=np.int32)
    idx[sys_.cells] = np.arange(sys_.size)
    diver = np.zeros(n ** 3, dtype=np.float32); diver[sys_.cells] = b
    pres = np.zeros(n ** 3); pres[sys_.cells] = p
    s2, res = ps.check_field_solve(sys_.solid, flags, idx, diver, pres, sys_.scale)
    assert np.array_equal(s2.count, sys_.count) and (sys_.count < 6).any() and res["eta"] < ps.ETA_BAR
    flags[sys_.cells[0]] ^= 4
    with pytest.raises(AssertionError, match="count bits"):
        ps.check_field_solve(sys_.solid, flags, idx, diver, pres, sys_.scale)
    flags[sys_.cells[0]] ^= 4
    pres[np.flatnonzero(idx < 0)[n * n + n + 1]] = 1e-300
    with pytest.raises(AssertionError, match="outside"):
        ps.check_field_solve(sys_.solid, flags, idx, diver, pres, sys_.scale)


def test_residual_is_exact(fs, oracle):
    """residual() against Fraction arithmetic on a ~500-unknown system: r exactly rounded, eta / omega / relres to the last bit."""
    n = 16
    o = oracle.Oracle(n=n)
    pos = fs.water_cube_drop(n, 3, seed=7)
    o.set_particles(pos, np.random.default_rng(3).standard_normal(pos.shape))
    o.p2g(); o.flags_index()
    sys_, _, b, p = _solved(oracle, o)
    assert 300 <= sys_.size <= 800, sys_.size
    res = ps.residual(sys_, b, p)
    F = Fraction
    off = F(sys_.off)
    rx, mx = [], []
    for i in range(sys_.size):
        ri = F(b[i]) - F(sys_.diag[i]) * F(p[i])
        mi = abs(F(b[i])) + abs(F(sys_.diag[i]) * F(p[i]))
        for j in sys_.nb[i]:
            if j >= 0:
                ri -= off * F(p[j])
                mi += abs(off * F(p[j]))
        rx.append(ri)
        mx.append(mi)
    # every r_i to within the long double's own rounding of a value with ~64 correct bits
    for i in range(sys_.size):
        assert abs(F(float(res["r"][i])) - rx[i]) <= abs(rx[i]) * F(1, 2 ** 52), i
    decimal.getcontext().prec = 60
    D = lambda f: decimal.Decimal(f.numerator) / decimal.Decimal(f.denominator)   # noqa: E731
    nr2, nm2, nb2 = sum(x * x for x in rx), sum(x * x for x in mx), sum(F(x) * F(x) for x in b)
    eta = float((D(nr2) / D(nm2)).sqrt())
    relres = float((D(nr2) / D(nb2)).sqrt())
    omega = float(D(max(abs(r) / m for r, m in zip(rx, mx))))
    print(f"exact eta {eta!r} omega {omega!r} relres {relres!r}; long double {res['eta']!r} {res['omega']!r} {res['relres']!r}")
    assert res["eta"] == eta and res["omega"] == omega and res["relres"] == relres
    o.close()


def _eigen(oracle, rows, cols, vals, b):
    if oracle.ref_lib() is None:
        return None
    x, _, _ = oracle.eigen_icpcg(len(b), rows, cols, vals, b)
    return x


@pytest.mark.parametrize("name", SCENES)
def test_calibration_sits_under_the_bars(oracle, systems, name):
    """The bars are justified by what converged fp64 CGs reach on these systems: both at least 4x under them."""
    sys_, (rows, cols, vals), b, p = systems[name]
    res = ps.residual(sys_, b, p)
    line = f"{name}: n_unknowns {sys_.size} oracle CG eta {res['eta']:.2e} omega {res['omega']:.2e} relres {res['relres']:.2e}"
    worst = [res]
    x = _eigen(oracle, rows, cols, vals, b)
    if x is not None:
        rx = ps.residual(sys_, b, x)
        line += f" | Eigen IC-PCG eta {rx['eta']:.2e} omega {rx['omega']:.2e}"
        worst.append(rx)
    print(line)
    for r in worst:
        assert 4 * r["eta"] <= ps.ETA_BAR, line
        assert 4 * r["omega"] <= ps.OMEGA_BAR, line


def test_perturbations_fail_the_bars(systems):
    """The bars can fail: p perturbed by 1e-14 relative (random signs) misses eta; one cell moved by 1e-13 misses omega."""
    sys_, _, b, p = systems["pool30"]
    assert ps.residual(sys_, b, p)["eta"] <= ps.ETA_BAR
    rng = np.random.default_rng(0)
    pe = p * (1 + 1e-14 * rng.choice([-1.0, 1.0], size=p.size))
    re = ps.residual(sys_, b, pe)
    print(f"1e-14 relative perturbation: eta {re['eta']:.2e} omega {re['omega']:.2e}")
    assert re["eta"] > ps.ETA_BAR
    k = int(np.argmax(np.abs(p)))
    pc = p.copy()
    pc[k] *= 1 + 1e-13
    rc = ps.residual(sys_, b, pc)
    print(f"one cell by 1e-13: eta {rc['eta']:.2e} omega {rc['omega']:.2e}")
    assert rc["omega"] > ps.OMEGA_BAR


def test_components_split_the_residual(systems):
    """components() on a split of the rows: each part's eta / omega are residual()'s restricted to it; the max omega is the whole's."""
    sys_, _, b, p = systems["blobs"]
    comp = np.full((2, sys_.size), -1, dtype=np.int64)
    half = sys_.size // 2
    comp[0, :half] = sys_.cells[:half]
    comp[1, :sys_.size - half] = sys_.cells[half:]
    parts = ps.components(sys_, b, p, comp)
    whole = ps.residual(sys_, b, p)
    assert max(c["omega"] for c in parts) == whole["omega"]
    assert np.array_equal(np.sort(np.concatenate([c["rows"] for c in parts])), np.arange(sys_.size))
