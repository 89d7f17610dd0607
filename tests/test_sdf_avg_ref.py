"""CPU (-m "not gpu"): the averaged-position surface (include/fluid_hip.h, "liquid surface, averaged positions") on its numpy
reference alone (tests/sdf_avg_ref.py): what the definition promises, before any library code is asked for it."""
import numpy as np
import pytest

import sdf_avg_ref
import sdf_ref
from sdf_avg_ref import block_and_scattered
from sdf_testlib import u32


def pool(n=24, ppc=8, seed=7):
    """ppc particles per cell in the lower half of the box."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    rng = np.random.default_rng(seed)
    c = np.stack(np.meshgrid(np.arange(lo, hi + 1), np.arange(lo, hi + 1), np.arange(lo, 0), indexing="ij"), axis=-1).reshape(-1, 3)
    return np.repeat(c, ppc, axis=0) + rng.uniform(-0.5, 0.5, (ppc * len(c), 3))


def crossing_heights(val, n, cols):
    """The height at which each column's values first turn from negative to non-negative going up, by linear interpolation."""
    lo = sdf_ref.geometry(n)[0]
    out = []
    for ix, iy in cols:
        v = val[ix - lo, iy - lo].astype(np.float64)
        k = int(np.flatnonzero((v[:-1] < 0) & (v[1:] >= 0))[0])
        out.append(lo + k + v[k] / (v[k] - v[k + 1]))
    return np.array(out)


@pytest.fixture(scope="module")
def scene():
    n, (R, w, dx, h) = 24, (1.0, 3.0, 1.0, 3.0)
    pos = block_and_scattered(n)
    return n, (R, w, dx, h), pos, sdf_avg_ref.averaged(pos, n, R, w, dx, h), sdf_ref.closed(pos, n, R, w, dx)


def test_a_permutation_gives_identical_bytes(scene):
    n, (R, w, dx, h), pos, (val, act), _ = scene
    perm = np.random.default_rng(1).permutation(len(pos))
    v2, a2 = sdf_avg_ref.averaged(pos[perm], n, R, w, dx, h)
    assert v2.tobytes() == val.tobytes() and a2.tobytes() == act.tobytes()


def test_never_outside_the_spheres(scene):
    """d >= ds: the active set is a subset of the spheres', and no active value lies below theirs."""
    _, _, _, (val, act), (sval, sact) = scene
    assert act.any() and not (act & ~sact).any()
    assert (val[act] >= sval[act]).all()
    assert np.array_equal(u32(val[~sact]), u32(sval[~sact]))           # what the spheres leave inactive stays what it was
    assert (u32(val) != u32(sval)).any()                                # and it is another surface


@pytest.mark.parametrize("p", [[1.0, -2.0, 3.0], [0.3, -1.7, 2.25], [1.5, -2.5, 0.5]])
def test_one_particle_is_a_sphere(p):
    """The average of one position is that position, up to the offset's quantum (2^-19 voxel per axis) and a few float ulps at 4:
    masks equal to the spheres', values within 1e-5 dx."""
    n, (R, w, dx, h) = 16, (1.5, 2.5, 0.5, 4.0)
    pos = np.array([p])
    val, act = sdf_avg_ref.averaged(pos, n, R, w, dx, h)
    sval, sact = sdf_ref.closed(pos, n, R, w, dx)
    assert act.any() and np.array_equal(act, sact)
    err = np.abs(val.astype(np.float64) - sval).max()
    print(f"one particle {p}: max |averaged - spheres| = {err:.3g} (dx = {dx})")
    assert err <= 1e-5 * dx


def test_a_gap_between_two_slabs_stays_open():
    """Two slabs 4.5 voxels apart, h = 3: the plain average fills the gap (negative at its middle), the maximum with the spheres'
    distance keeps it open."""
    n, (R, w, dx, h) = 16, (1.0, 3.0, 1.0, 3.0)
    lo = sdf_ref.geometry(n)[0]
    g = np.arange(-7.75, 8.0, 0.5)
    zs = np.concatenate([np.arange(-5.25, -2.0, 0.5), np.arange(2.25, 5.5, 0.5)])
    pos = np.stack(np.meshgrid(g, g, zs, indexing="ij"), axis=-1).reshape(-1, 3)
    assert zs[zs > 0].min() - zs[zs < 0].max() == 4.5
    m, SW, SX, SY, SZ = sdf_avg_ref.sums(pos, n, h)
    val, act = sdf_avg_ref.finish(m, SW, SX, SY, SZ, R, w, dx)
    c = (-lo, -lo, -lo)                                                                         # voxel (0, 0, 0): the middle of the gap
    a = np.array([SX[c], SY[c], SZ[c]], dtype=np.float64) / (float(SW[c]) * 262144.0)
    plain = dx * (np.linalg.norm(a) - R)
    print(f"gap: plain average {plain:.3f}, with the spheres' distance {val[c]:.3f}")
    assert SW[c] > 0 and plain < 0
    assert act[c] and val[c] > 0


def test_a_pool_is_flatter_than_its_spheres():
    """8 particles per cell in the lower half of a 24^3 box, R = 1, w = 3, h = 3: the height of the zero crossing over the 144
    columns in the middle varies less than the spheres' (the figures: profiles/avg/NOTES.md; no ratio is asserted)."""
    n, (R, w, dx, h) = 24, (1.0, 3.0, 1.0, 3.0)
    pos = pool(n)
    cols = [(x, y) for x in range(-6, 6) for y in range(-6, 6)]
    ha = crossing_heights(sdf_avg_ref.averaged(pos, n, R, w, dx, h, set(cols))[0], n, cols)
    hs = crossing_heights(sdf_ref.closed(pos, n, R, w, dx)[0], n, cols)
    print(f"pool, {len(cols)} columns: std of the crossing height {ha.std():.4f} averaged, {hs.std():.4f} spheres; "
          f"range {np.ptp(ha):.3f} against {np.ptp(hs):.3f}; mean {ha.mean():.3f} against {hs.mean():.3f}")
    assert ha.std() < hs.std()
