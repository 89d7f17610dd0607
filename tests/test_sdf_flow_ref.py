"""CPU (-m "not gpu"): known answers of the numpy reference of the liquid surface's flows (tests/sdf_flow_ref.py) itself: fixed
points of the Laplacian and the curvature flow, the key order of the median at the two zeros, the direction of curvature flow on a
sphere, and kind = BOX against tests/sdf_filter_ref.py and its tracked and grown forms."""
import numpy as np

import sdf_filter_ref
import sdf_flow_ref as R
import sdf_grow_ref as G
import sdf_ref
import sdf_track_ref
from sdf_testlib import u32

F = np.float32


def test_a_dyadic_plane_is_a_fixed_point_of_laplacian_and_curvature():
    """val = 0.5 x + 0.25 with dx = 1: every difference is exact, the Laplacian and the curvature term are +0.  Away from the pad
    (which is +bg, no plane) every active voxel keeps its bytes."""
    n, dx, bg = 12, 1.0, F(100.0)
    x = np.arange(n, dtype=F)[:, None, None]
    val = np.broadcast_to(F(0.5) * x + F(0.25), (n, n, n)).astype(F)
    act = np.zeros((n, n, n), bool)
    act[1:-1, 1:-1, 1:-1] = True
    for kind in (R.LAPLACIAN, R.CURVATURE):
        out = R.flow_pass(kind, val, act, bg, dx, 1)
        assert np.array_equal(u32(out), u32(val)), kind
        out = R.flow(kind, val, act, bg, dx, 1, 3)[0]
        assert np.array_equal(u32(out), u32(val)), kind
    # a tilted dyadic plane as well: the mixed differences cancel exactly
    y = np.arange(n, dtype=F)[None, :, None]
    z = np.arange(n, dtype=F)[None, None, :]
    val = (F(0.5) * x + F(0.25) * y - F(0.125) * z + F(0.25)).astype(F)
    for kind in (R.LAPLACIAN, R.CURVATURE):
        assert np.array_equal(u32(R.flow_pass(kind, val, act, bg, dx, 1)), u32(val)), kind


def test_the_plateau_is_a_fixed_point():
    """All +bg or all -bg, every voxel active: ng = 0, the curvature term is the constant 0.0f; the Laplacian's sum is exact."""
    n, dx = 8, 0.5
    act = np.ones((n, n, n), bool)
    bg = F(1.0)
    val = np.full((n, n, n), bg, F)
    for kind, W in R.CASES:
        assert np.array_equal(u32(R.flow_pass(kind, val, act, bg, dx, W)), u32(val)), kind
    neg = np.full((n, n, n), -bg, F)
    inner = np.zeros((n, n, n), bool)
    inner[2:-2, 2:-2, 2:-2] = True   # (the pad is +bg: only voxels whose stencil stays inside see the -bg plateau alone)
    for kind, W in R.CASES:
        assert np.array_equal(u32(R.flow_pass(kind, neg, inner, bg, dx, W)), u32(neg)), kind


def test_the_median_key_order_decides_between_the_zeros():
    """27 values: 12 negative, then -0 and +0, then 13 positive: rank 13 is +0, and with one negative more it is -0."""
    neg, pos = -np.arange(1, 13, dtype=F), np.arange(1, 14, dtype=F)
    a = np.concatenate([neg, [F(-0.0), F(0.0)], pos]).astype(F)
    assert len(a) == 27
    rng = np.random.default_rng(5)
    for _ in range(4):
        assert u32(R.median_of(rng.permutation(a))) == u32(F(0.0))            # ranks: 12 negatives, -0 at 12, +0 at 13
    b = np.concatenate([neg, [F(-13.0)], [F(-0.0), F(0.0)], pos[:-1]]).astype(F)
    for _ in range(4):
        assert u32(R.median_of(rng.permutation(b))) == u32(F(-0.0))           # 13 negatives: -0 at 13
    k = R.keys(np.array([-np.inf, -2.0, -0.0, 0.0, 1e-45, 3.0, np.inf], F))
    assert (np.diff(k.astype(np.int64)) > 0).all() and np.array_equal(u32(R.unkeys(k)), u32(np.array([-np.inf, -2.0, -0.0, 0.0, 1e-45, 3.0, np.inf], F)))
    # through a pass: the centre voxel of a 3^3 grid holding b, all active
    val = rng.permutation(b).reshape(3, 3, 3)
    out = R.median_pass(val, np.ones((3, 3, 3), bool), F(50.0), 1)
    assert u32(out[1, 1, 1]) == u32(F(-0.0))


def test_curvature_flow_shrinks_a_sphere():
    """One sphere, R = 3, w = 1: after 4 tracked curvature iterations strictly fewer voxels are inside.  Direction only."""
    n, Rad, w, dx = 16, 3.0, 1.0, 1.0
    val, act = sdf_ref.closed(np.array([[0.3, -0.2, 0.41]]), n, Rad, w, dx)
    bg = sdf_ref.constants(Rad, w, dx)[3]
    before = int((val < 0).sum())
    out = R.flow(R.CURVATURE, val, act, bg, dx, 1, 4, 0.0, 3, True)[0]
    after = int((out < 0).sum())
    assert 0 < after < before, (before, after)


def test_kind_box_is_the_box_filter():
    n, Rad, w, dx = 16, 2.0, 2.0, 1.0
    _, val, act, ids, v32, bg = R.base("cloud", n, Rad, w, dx)
    for W, K, off in [(1, 1, 0.0), (2, 2, 0.5), (1, 0, -0.25)]:
        out = R.flow(R.BOX, val, act, bg, dx, W, K, off)
        assert np.array_equal(u32(out[0]), u32(sdf_filter_ref.smooth(val, act, bg, W, K, off))) and np.array_equal(out[1], act)
    vt, at = sdf_track_ref.tracked(val, act, bg, dx, 1, 2, 0.6, 3, True)
    out = R.flow(R.BOX, val, act, bg, dx, 1, 2, 0.6, 3, True)
    assert np.array_equal(u32(out[0]), u32(vt)) and np.array_equal(out[1], at)
    vg, ag, ig, velg = G.grown(val, act, bg, dx, 1, 1, -3.0, 3, ids, v32)
    out = R.flow(R.BOX, val, act, bg, dx, 1, 1, -3.0, 3, True, True, ids, v32)
    assert np.array_equal(u32(out[0]), u32(vg)) and np.array_equal(out[1], ag) and np.array_equal(out[2], ig) and np.array_equal(u32(out[3]), u32(velg))
