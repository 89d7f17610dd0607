"""CPU (-m "not gpu"): properties of the HJWENO5 definition (include/fluid_hip.h, "liquid surface, renormalised: HJWENO5"), checked
on the numpy reference tests/sdf_weno_ref.py alone, so that a mis-restated stencil cannot hide behind three implementations that
agree: the two exact symmetries of the biased differences and of the voxel function, linear data, the drift of an exact sphere
against the first-order reference's (the yardstick is sdf_track_ref, not the code under test), and sign, finiteness and mesh counts
over the scenes and cases of sdf_track_ref.  What these properties cannot see — a weight order, a pass order, a rounding point — is
pinned by tests/test_vdb_ref.py, which compares the same functions bit for bit with OpenVDB's own lines compiled in place.

Measured with this file (max |val - d| over active |d| < 1.5 after track(3), dx = 1; FIRST_BIAS / HJWENO5 / ratio):
  R = 4: 0.09581 / 0.00116 / 82.7      R = 6: 0.06529 / 0.00071 / 91.4      R = 9: 0.04470 / 0.00037 / 122.1
and after an offset of +-0.5 and one track, against d + off over |d + off| < 1.5, R = 4, 6, 9 (the smallest ratio is 10.4):
  +0.5: 0.12119 / 0.00305,  0.07474 / 0.00125,  0.04569 / 0.00101      -0.5: 0.08471 / 0.00816,  0.06087 / 0.00251,  0.04203 / 0.00275
"""
import numpy as np
import pytest

import mesh_ref
import sdf_filter_ref
import sdf_track_ref
import sdf_weno_ref as W
from sdf_testlib import u32

F = np.float32


def septuples(count, seed):
    """count random septuples (7, count): smooth ones, rough ones, clamped ones, and tiny ones."""
    rng = np.random.default_rng(seed)
    k = np.arange(-3, 4, dtype=np.float64)[:, None]
    q = count // 4
    smooth = rng.uniform(-2, 2, q) + rng.uniform(-1.2, 1.2, q) * k + rng.uniform(-0.1, 0.1, q) * k * k
    rough = rng.uniform(-3, 3, (7, q))
    clamped = np.clip(rng.uniform(-1, 1, q) + rng.uniform(0.5, 1.5, q) * k, -2.5, 2.5)
    tiny = rng.uniform(-1, 1, (7, count - 3 * q)) * 1e-20
    return np.concatenate([smooth, rough, clamped, tiny], axis=1).astype(F)


def test_differences_obey_the_two_symmetries_bit_for_bit():
    u = septuples(1000, 1)
    dm, dp = W.axis_diffs(list(u))
    assert np.isfinite(dm).all() and np.isfinite(dp).all()
    nm, np_ = W.axis_diffs(list(-u))
    assert np.array_equal(u32(nm), u32(-dm)) and np.array_equal(u32(np_), u32(-dp))
    rm, rp = W.axis_diffs(list(u[::-1]))
    assert np.array_equal(u32(rm), u32(-dp)) and np.array_equal(u32(rp), u32(-dm))
    assert len(np.unique(u32(dm))) > 900 and (u32(dm) != u32(dp)).sum() > 500          # the check is not vacuous


@pytest.mark.parametrize("b", [0.0, 1.0, -2.0, 0.3, -0.7, 1e-3])
def test_linear_data_gives_its_slope(b):
    rng = np.random.default_rng(2)
    a = rng.uniform(-3, 3, 200)
    k = np.arange(-3, 4, dtype=np.float64)[:, None]
    u = (a + b * k).astype(F)
    dm, dp = W.axis_diffs(list(u))
    # each value is rounded at size <= 3 + 3 |b|, so each difference is b within one spacing s of that size; W5 is a convex combination
    # of three stencils whose coefficients sum to 20/6 in magnitude at most: 3.34 s, and the result's own rounding
    tol = 4 * np.spacing(F(3 + 3 * abs(b)))
    assert np.abs(dm.astype(np.float64) - b).max() <= tol and np.abs(dp.astype(np.float64) - b).max() <= tol
    if b in (0.0, 1.0, -2.0):   # exactly representable steps from a = 0: the differences are exact, so the slope is b within an ulp
        e = [F(b * i) for i in range(-3, 4)]
        em, ep = W.axis_diffs(e)
        assert abs(float(em) - b) <= np.spacing(F(abs(b))) and abs(float(ep) - b) <= np.spacing(F(abs(b)))


def test_voxel_function_obeys_the_two_symmetries():
    count = 1000
    ux, uy, uz = septuples(count, 3), septuples(count, 4), septuples(count, 5)
    p = ux[3].copy()
    assert (p != 0).all()
    uy[3], uz[3] = p, p
    dx = F(0.8)
    v = W.voxel_value(ux, uy, uz, dx)
    assert np.isfinite(v).all() and (u32(v) != u32(p)).sum() > 900
    assert np.array_equal(u32(W.voxel_value(-ux, -uy, -uz, dx)), u32(-v))                    # negation
    assert np.array_equal(u32(W.voxel_value(ux[::-1], uy[::-1], uz[::-1], dx)), u32(v))      # reflection: (-dp, -dm) feeds the same term


def sphere_figures(R):
    val, act, d = W.sphere(R)
    out = {}
    for scheme in (W.FIRST, W.HJWENO5):
        v, a = W.track(val, act, W.SPHERE_BG, 1.0, 3, True, scheme)
        out[scheme] = W.drift(v, a, d)
    return out


@pytest.mark.parametrize("R", W.SPHERE_RADII)
def test_an_exact_sphere_drifts_a_tenth_of_first_order_at_most(R):
    e = sphere_figures(R)
    print(f"R={R}: first {e[W.FIRST]:.5f} hjweno5 {e[W.HJWENO5]:.5f} ratio {e[W.FIRST] / e[W.HJWENO5]:.1f}")
    assert e[W.FIRST] > 0.03                                  # the yardstick is what the issue measured: a real drift
    assert e[W.HJWENO5] <= e[W.FIRST] / 10


@pytest.mark.parametrize("off", [0.5, -0.5])
@pytest.mark.parametrize("R", W.SPHERE_RADII)
def test_an_offset_sphere_drifts_a_fifth_of_first_order_at_most(R, off):
    val, act, d = W.sphere(R)
    e = {}
    for scheme in (W.FIRST, W.HJWENO5):
        v = np.where(act, val + F(off), val)
        assert v.dtype == F
        v, a = W.track(v, act, W.SPHERE_BG, 1.0, 3, True, scheme)
        m = a & (np.abs(d + off) < 1.5)
        e[scheme] = float(np.abs(v.astype(np.float64)[m] - (d + off)[m]).max())
    print(f"R={R} off={off}: first {e[W.FIRST]:.5f} hjweno5 {e[W.HJWENO5]:.5f} ratio {e[W.FIRST] / e[W.HJWENO5]:.1f}")
    assert e[W.HJWENO5] <= e[W.FIRST] / 5


@pytest.mark.parametrize("R,w,dx", mesh_ref.SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", ["one", "corner", "lo", "hi", "cloud"])
def test_no_pass_changes_a_sign_and_counts_stay(name, n, R, w, dx):
    _, val, act, bg, _ = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))
    for Wd, K, units, N, tr in sdf_track_ref.TRACKS:
        v = np.array(val)
        for _ in range(K):
            for a in sdf_filter_ref.ORDER:
                v = sdf_filter_ref.box_pass(v, act, bg, Wd, a)
        for _ in range(N):
            nxt = W.norm_pass_weno(v, act, bg, dx)
            assert np.isfinite(nxt).all()
            assert np.array_equal(nxt > 0, v > 0) and np.array_equal(nxt < 0, v < 0), (name, n, Wd, K, N)
            assert np.array_equal(u32(nxt[~act]), u32(v[~act]))
            v = nxt
        vt, at = W.tracked(val, act, bg, dx, Wd, K, units * dx, N, bool(tr))
        assert np.isfinite(vt).all()
        if K == 1 and units == 0.0:   # the mesh of the tracked field has the untracked filtered mesh's counts
            plain = mesh_ref.mesh(sdf_filter_ref.smooth(val, act, bg, Wd, K, 0.0))
            m = mesh_ref.mesh(vt)
            assert m[0].shape == plain[0].shape and m[1].shape == plain[1].shape, (name, n, Wd, K, N)
