"""CPU (-m "not gpu"): the numpy reference of the velocity trails (tests/sdf_trail_ref.py) on its own: a known answer, the cases
in which the trails are the spheres of sdf_ref.closed() bit for bit, the two ways in which a radius per item differs from a
minimum of squared distances, the exact split over a partition of the items, and that no order is involved."""
import numpy as np
import pytest

import sdf_ref
import sdf_trail_ref as ref
from sdf_testlib import u32

F = np.float32


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))


def test_known_answer():
    """R = 2, Rm = 1, delta = 1, shutter * |v| = 3 along +x: t = 0, 1, 1 + 5/6, ... behind the particle."""
    P, r, who = ref.instances([[0.5, 0.25, -1.0]], [[1.5, 0.0, 0.0]], 2.0, (2.0, 1.0, 1.0, 16))
    assert len(P) == 4 and who.tolist() == [0] * 4
    t = np.array([0.0, 1.0, 1.0 + 5.0 / 6.0, 1.0 + 5.0 / 6.0 + 25.0 / 36.0])
    assert np.abs(t - [0, 1, 1.8333333, 2.5277778]).max() < 1e-6
    assert np.abs(P[:, 0] - (0.5 - t)).max() <= 1e-6 and (P[:, 1] == 0.25).all() and (P[:, 2] == -1.0).all()
    assert P[0].tolist() == [0.5, 0.25, -1.0] and r[0] == F(2.0)
    assert np.abs(r - [2.0, 1.6666667, 1.3888889, 1.1574074]).max() <= 1e-6
    P3, r3, _ = ref.instances([[0.5, 0.25, -1.0]], [[1.5, 0.0, 0.0]], 2.0, (2.0, 1.0, 1.0, 3))
    assert len(P3) == 3 and np.array_equal(P3, P[:3]) and np.array_equal(r3, r[:3])
    assert len(ref.instances([[0.5, 0.25, -1.0]], [[1.5, 0.0, 0.0]], 2.0, (2.0, 1.0, 1.0, 1))[0]) == 1


@pytest.mark.parametrize("R,w,dx", ref.SETS)
def test_no_motion_is_the_spheres(R, w, dx):
    n = 16
    rng = np.random.default_rng(1)
    pos = rng.uniform(-9.0, 9.0, (60, 3))
    closed = sdf_ref.closed(pos, n, R, w, dx)
    vel = rng.normal(size=pos.shape)
    for name, v, shutter in (("zero", np.zeros_like(pos), 1.0), ("nan", np.full_like(pos, np.nan), 1.0), ("inf", np.full_like(pos, np.inf), 1.0),
                             ("-inf on one axis", vel * np.array([1.0, -np.inf, 1.0]), 1.0), ("overflow", vel * 1e200, 1e200),
                             ("shutter 0", vel, 0.0)):
        P, r, who = ref.instances(pos, v, R, (shutter, 1.0, R / 2, 8))
        assert len(P) == len(pos) and np.array_equal(P, pos) and (r == F(R)).all() and np.array_equal(who, np.arange(len(pos))), name
        assert same(ref.union(P, r, n, R, w, dx), closed), name
    assert closed[1].any()


@pytest.mark.parametrize("R,w,dx", ref.SETS)
def test_constant_radius_is_the_spheres_of_the_instances(R, w, dx):
    n = 16
    rng = np.random.default_rng(2)
    pos = rng.uniform(-9.0, 9.0, (40, 3))
    vel = rng.normal(size=pos.shape) * 3.0
    P, r, _ = ref.instances(pos, vel, R, (1.0, 1.0, R, 8))
    assert len(P) > 2 * len(pos) and (r == F(R)).all()
    assert same(ref.union(P, r, n, R, w, dx), sdf_ref.closed(P, n, R, w, dx))


def test_a_farther_larger_item_wins_the_value():
    """Voxel 0: the item at distance 2.5 with radius 2 gives d = 0.5, the nearer one at distance 2.0 with radius 1 gives d = 1."""
    n, R, w, dx = 16, 2.0, 2.0, 1.0
    lo = sdf_ref.geometry(n)[0]
    o = (-lo, -lo, -lo)
    items, radii = np.array([[2.5, 0.0, 0.0], [-2.0, 0.0, 0.0]]), np.array([2.0, 1.0], dtype=F)
    val, act = ref.union(items, radii, n, R, w, dx)
    assert act[o] and val[o] == F(0.5)
    assert ref.union(items[1:], radii[1:], n, R, w, dx)[0][o] == F(1.0)
    # with one radius the nearer item decides
    assert sdf_ref.closed(items, n, R, w, dx)[0][o] == F(0.0)


def test_a_large_item_makes_a_voxel_inside_although_a_small_one_is_nearer():
    n, R, w, dx = 16, 3.0, 1.0, 1.0
    lo = sdf_ref.geometry(n)[0]
    o = (-lo, -lo, -lo)
    items, radii = np.array([[1.5, 0.0, 0.0], [-1.0, 0.0, 0.0]]), np.array([3.0, 1.0], dtype=F)
    bg = sdf_ref.constants(R, w, dx)[3]
    val, act = ref.union(items, radii, n, R, w, dx)
    assert not act[o] and val[o] == -bg
    v1, a1 = ref.union(items[1:], radii[1:], n, R, w, dx)
    assert a1[o] and v1[o] == F(0.0)
    for order in ([0, 1], [1, 0]):
        assert same(ref.union(items[order], radii[order], n, R, w, dx), (val, act))


@pytest.mark.parametrize("R,w,dx", ref.SETS)
def test_union_splits_over_a_partition_and_knows_no_order(R, w, dx):
    """union(A + B) is the rule of fluid_sdf_grids_merge applied to union(A) and union(B): rank lists of trails would merge exactly."""
    n = 16
    rng = np.random.default_rng(3)
    pos = np.vstack([rng.uniform(-9.0, 9.0, (50, 3)), rng.uniform(-1.5, 1.5, (150, 3))])
    vel = rng.normal(size=pos.shape) * 2.5
    P, r, _ = ref.instances(pos, vel, R, ref.trails_of(R))
    assert len(P) > len(pos) and r.min() < F(R)
    whole = ref.union(P, r, n, R, w, dx)
    bg = sdf_ref.constants(R, w, dx)[3]
    part = rng.random(len(P)) < 0.5
    assert same(ref.merge(ref.union(P[part], r[part], n, R, w, dx), ref.union(P[~part], r[~part], n, R, w, dx), bg), whole)
    o = rng.permutation(len(P))
    assert same(ref.union(P[o], r[o], n, R, w, dx), whole)
    assert (whole[0][~whole[1]] < 0).any() == (R > w)
