"""CPU (-m "not gpu"): the reference of the liquid surface checks itself — the closed form over the minimum squared distance
(tests/sdf_ref.py closed(), what the kernels are held to) against the particle-by-particle restatement of OpenVDB's
rasterFixedSpheres (sequential()), values bit for bit and masks, in two particle orders."""
import numpy as np
import pytest

import sdf_ref
from sdf_testlib import u32

# (R, w, dx); the first has R + w > 4: refused by the C ABI, valid for the reference
SETS = [(1.5, 3.0, 1.0), (1.5, 2.5, 1.0), (3.0, 1.0, 1.0), (1.0, 2.0, 0.5), (2.0, 2.0, 1.0)]
N = 16


def particles():
    rng = np.random.default_rng(7)
    lo, hi, _, _ = sdf_ref.geometry(N)
    p = rng.uniform(lo - 1.0, hi + 1.0, size=(60, 3))      # a few have their base cell outside the grid
    p[:20] = rng.uniform(-3.0, 3.0, size=(20, 3))           # a clump: voxels deep inside (m <= min2 when R > w)
    return np.vstack([p, [[2.0, -3.0, 1.0]]])                # one exactly on a voxel


@pytest.mark.parametrize("R,w,dx", SETS)
def test_closed_form_is_the_sequential_raster(R, w, dx):
    pos = particles()
    cv, ca = sdf_ref.closed(pos, N, R, w, dx)
    for order in (pos, pos[::-1]):
        sv, sa = sdf_ref.sequential(order, N, R, w, dx)
        assert np.array_equal(sa, ca)
        assert np.array_equal(u32(sv), u32(cv))
    _, _, _, bg, _, min2 = sdf_ref.constants(R, w, dx)
    assert ca.any() and (cv[~ca] == bg).any()
    assert np.array_equal((cv == -bg) & ~ca, sdf_ref.min_dist2(pos, N, 6) <= min2)
    lo = sdf_ref.geometry(N)[0]
    i = (2 - lo, -3 - lo, 1 - lo)
    assert cv[i] == -bg and not ca[i]                        # on the particle: m = 0 <= min2, whatever R and w


def test_constants_and_rounding():
    R, w, dxf, bg, max2, min2 = sdf_ref.constants(1.0, 2.0, 0.5)
    assert (bg, max2, min2) == (1.0, 9.0, 0.0)
    R, w, dxf, bg, max2, min2 = sdf_ref.constants(3.0, 1.0, 1.0)
    assert (bg, max2, min2) == (1.0, 16.0, 4.0)
    assert sdf_ref.base_cell([0.5, -0.5, 1.5, -1.5, 2.4999999999999996, 0.49999999999999994]).tolist() == [1, -1, 2, -2, 2, 0]


def test_leaf_list_layout():
    n = 25
    lo, hi, l0, nl = sdf_ref.geometry(n)
    bg = np.float32(2.5)
    val = np.full((n, n, n), bg, np.float32)
    act = np.zeros((n, n, n), bool)
    val[0, 0, 0], act[0, 0, 0] = 0.25, True
    val[n - 1, n - 1, n - 1] = -bg
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert org.tolist() == [[l0] * 3, [hi & ~7] * 3]
    off0 = ((lo - l0) * 8 + (lo - l0)) * 8 + (lo - l0)
    assert v[0, off0] == 0.25 and a[0, off0] and a.sum() == 1 and (np.delete(v[0], off0) == bg).all()
    off1 = (((hi & 7) * 8) + (hi & 7)) * 8 + (hi & 7)
    assert v[1, off1] == -bg and not a[1].any()
