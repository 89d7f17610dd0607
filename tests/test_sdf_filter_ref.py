"""CPU (-m "not gpu"): the numpy reference of the smoothed liquid surface (tests/sdf_filter_ref.py) against its definition
(include/fluid_hip.h, "liquid surface, smoothed"): identity, inactive voxels, values computed by hand, the axis order."""
import numpy as np

import mesh_ref
import sdf_filter_ref as R
from sdf_testlib import u32

F = np.float32


def cloud():
    _, val, act, _ = mesh_ref.scene("cloud", 25, 3.0, 1.0, 1.0)
    return val, act, F(1.0)


def test_no_iteration_and_no_offset_is_the_identity():
    val, act, bg = cloud()
    for W in (1, 4):
        assert np.array_equal(u32(R.smooth(val, act, bg, W, 0, 0.0)), u32(val))
        assert np.array_equal(u32(R.smooth(val, act, bg, W, 0, -0.0)), u32(val))


def test_inactive_voxels_never_change():
    val, act, bg = cloud()
    assert (~act).any() and act.any() and (val[~act] == -bg).any() and (val[~act] == bg).any()
    for W, K, off in R.FILTERS + [(2, 3, -0.7)]:
        out = R.smooth(val, act, bg, W, K, off)
        assert np.array_equal(u32(out[~act]), u32(val[~act])), (W, K, off)
        if K > 0 or off != 0:
            assert not np.array_equal(u32(out[act]), u32(val[act])), (W, K, off)


def line_grid(n=16, bg=2.0):
    """+bg everywhere; along x at (., 5, 6): index 7 inactive -bg, index 8 ACTIVE 0.5, index 9 (and everything else) inactive +bg."""
    val = np.full((n, n, n), F(bg), F)
    act = np.zeros((n, n, n), bool)
    val[7, 5, 6] = -F(bg)
    val[8, 5, 6], act[8, 5, 6] = F(0.5), True
    return val, act, F(bg)


def test_hand_computed_width_1():
    val, act, bg = line_grid()
    third = F(1) / F(3)
    one = R.box_pass(val, act, bg, 1, 0)
    # s = ((0 + -2) + 0.5) + 2 = 0.5 exactly; 0.5 * fl(1/3) is exact too (a power of two)
    assert one[8, 5, 6] == F(0.5) * third and float(one[8, 5, 6]) == 0.16666667163372040
    assert np.array_equal(np.delete(u32(one).ravel(), (8 * 16 + 5) * 16 + 6), np.delete(u32(val).ravel(), (8 * 16 + 5) * 16 + 6))
    # the whole iteration, scalar by scalar: x, then z, then y; the z and y neighbours are inactive +bg
    x = F(F(F(F(0) + -bg) + F(0.5)) + bg) * third
    z = F(F(F(F(0) + bg) + x) + bg) * third
    y = F(F(F(F(0) + bg) + z) + bg) * third
    out = R.smooth(val, act, bg, 1, 1)
    assert u32(out[8, 5, 6]) == u32(y)
    off = R.smooth(val, act, bg, 1, 1, -0.25)
    assert u32(off[8, 5, 6]) == u32(F(y + F(-0.25))) and np.array_equal(u32(off[~act]), u32(val[~act]))


def test_hand_computed_width_2():
    val, act, bg = line_grid()
    one = R.box_pass(val, act, bg, 2, 0)
    # indices 6 .. 10: +2, -2, 0.5, +2, +2 -> s = 4.5 exactly; fl(1/5) = 0.2f; 4.5 * 0.2f = 0.9000000134... lies above the midpoint 0.90000000596 of the floats
    # 0.89999997616 and 0.90000003576: it rounds up
    fifth = F(1) / F(5)
    assert float(fifth) == 0.20000000298023224
    assert one[8, 5, 6] == F(4.5) * fifth and float(one[8, 5, 6]) == 0.90000003576278687
    # at the grid's face the padding is +bg: the same voxel pattern moved to x index 0 .. 1 reads two padded values
    val2 = np.full((16, 16, 16), bg, F)
    act2 = np.zeros((16, 16, 16), bool)
    val2[0, 5, 6] = -bg
    val2[1, 5, 6], act2[1, 5, 6] = F(0.5), True
    assert R.box_pass(val2, act2, bg, 2, 0)[1, 5, 6] == F(4.5) * fifth


def test_the_axis_order_matters():
    val, act, bg = cloud()
    a = R.smooth(val, act, bg, 1, 1)
    b = R.smooth(val, act, bg, 1, 1, order=(0, 1, 2))
    assert R.ORDER == (0, 2, 1)
    assert not np.array_equal(u32(a), u32(b))
    assert np.array_equal(u32(a), u32(R.smooth(val, act, bg, 1, 1, order=(0, 2, 1))))
