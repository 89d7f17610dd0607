"""CPU (-m "not gpu"): the numpy reference of the renormalised liquid surface (tests/sdf_track_ref.py) against its own definition
— term and axis order and the stepped offset pinned in bits, the stated properties (no sign change per pass, equal mesh counts
for K = 1 without offset, finiteness, a gradient closer to 1), and that the shared case list holds the cases the GPU tests rely
on."""
import numpy as np
import pytest

import mesh_ref
import sdf_filter_ref
import sdf_ref
import sdf_track_ref as T
from sdf_testlib import u32

F = np.float32
SCENES = ["one", "corner", "lo", "hi", "cloud"]


def leaves(val, act, bg):
    return len(sdf_ref.leaf_list(val, act, bg)[0])


def test_term_and_axis_order_are_pinned():
    """A hand-made asymmetric 3 x 3 x 3 neighbourhood, all active, bg = 3, dx = 1: the centre's value by hand, step by step; its
    bits change when the axis sum runs z, y, x and when (dt * S) * (...) becomes dt * (S * (...))."""
    bg, dx = F(3), F(1)
    val = np.full((3, 3, 3), F(0.7), F)
    p = F(0.61)
    val[1, 1, 1] = p
    val[0, 1, 1], val[2, 1, 1] = F(-1.15), F(1.53)          # x: dm > 0 counts
    val[1, 0, 1], val[1, 2, 1] = F(0.93), F(0.56)           # y: dp < 0 counts
    val[1, 1, 0], val[1, 1, 2] = F(-0.32), F(0.518)         # z: both count, the larger square wins
    act = np.ones((3, 3, 3), bool)
    got = T.norm_pass(val, act, bg, dx)[1, 1, 1]
    tx = F(p - F(-1.15)) * F(p - F(-1.15))
    ty = F(F(0.56) - p) * F(F(0.56) - p)
    dm, dp = F(p - F(-0.32)), F(F(0.518) - p)
    tz = max(F(dm * dm), F(dp * dp))
    G = F(F(tx + ty) + tz)
    S = F(p / F(F(np.sqrt(F(F(p * p) + G))) + F(1e-8)))
    want = F(p - F(F(F(dx * F(0.3)) * S) * F(F(F(np.sqrt(G)) * F(1)) - F(1))))
    assert got.dtype == F and u32(got) == u32(want)
    assert F(dm * dm) > F(dp * dp) and G > 1                                     # the correction pulls towards 0
    assert 0 < got < p
    rev = T.norm_pass(val, act, bg, dx, axes=(2, 1, 0))[1, 1, 1]
    assoc = T.norm_pass(val, act, bg, dx, assoc=True)[1, 1, 1]
    assert u32(rev) != u32(got) and u32(assoc) != u32(got)
    assert abs(float(rev) - float(got)) < 1e-6 and abs(float(assoc) - float(got)) < 1e-6
    # inside (p < 0) the other one-sided differences count
    neg = T.norm_pass(-val, act, bg, dx)[1, 1, 1]
    assert u32(neg) == u32(-got)
    # an inactive voxel keeps its value; outside the array the pass reads +bg
    act2 = act.copy()
    act2[1, 1, 1] = False
    out = T.norm_pass(val, act2, bg, dx)
    assert u32(out[1, 1, 1]) == u32(p) and u32(out[0, 0, 0]) != u32(val[0, 0, 0])


def test_stepped_offset_is_pinned():
    """+0.6 dx is the steps 0.5 and 0.1 (float: 0.6f - 0.5f), each followed by a track: other bits than one step of 0.6."""
    for dx in (1.0, 0.5):
        steps = T.offset_steps(0.6 * dx, dx)
        assert len(steps) == 2 and steps[0] == F(0.5) * F(dx) and u32(steps[1]) == u32(F(F(0.6 * dx) - F(0.5) * F(dx)))
    assert T.offset_steps(-0.25, 1.0) == [F(-0.25)] and T.offset_steps(0.0, 1.0) == [] and T.offset_steps(0.0002, 1.0) == []
    assert [float(s) for s in T.offset_steps(-2.0, 1.0)] == [-0.5] * 4
    _, val, act, bg, _ = sdf_filter_ref.scene("cloud", 16, 2.0, 2.0, 1.0, (1, 0, 0.0))
    two, a2 = T.tracked(val, act, bg, 1.0, 1, 0, 0.6, 2, True)
    one, a1 = T.track(np.where(act, val + F(0.6), val), act, bg, 1.0, 2, True)
    assert not np.array_equal(u32(two), u32(one)) and a1.any() and a2.any()


@pytest.mark.parametrize("R,w,dx", mesh_ref.SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", SCENES)
def test_properties_on_every_scene(name, n, R, w, dx):
    """No pass changes a voxel's sign; everything stays finite; inactive voxels hold +-bg; the trim deactivates exactly the active
    voxels at or beyond +-bg; K = 1 without offset keeps the untracked mesh's vertex and quad counts."""
    _, val, act, bg, _ = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))
    for case in T.TRACKS:
        W, K, units, N, tr = case
        _, vt, at, _, mesh = T.scene(name, n, R, w, dx, case)
        assert vt.dtype == F and np.isfinite(vt).all(), case
        assert not (at & ~act).any(), case                                       # the band never grows
        assert (np.abs(vt[~at]) == bg).all(), case
        if tr:
            assert (np.abs(vt[at]) < bg).all(), case
        if N == 0 and not tr:
            sm = sdf_filter_ref.scene(name, n, R, w, dx, (W, K, units * dx))
            assert np.array_equal(u32(vt), u32(sm[1])) and np.array_equal(at, act), case
        if K == 1 and units == 0.0:
            plain = sdf_filter_ref.scene(name, n, R, w, dx, (W, K, 0.0))[4]
            assert len(mesh[0]) == len(plain[0]) and len(mesh[1]) == len(plain[1]), case
            if N > 0 and len(plain[0]) > 0:
                assert not np.array_equal(u32(mesh[0]), u32(plain[0])), case      # only positions move
    v = sdf_filter_ref.smooth(val, act, bg, 1, 1)
    for _ in range(3):                                                           # pass by pass after one box iteration
        nv = T.norm_pass(v, act, bg, dx)
        assert np.array_equal(nv < 0, v < 0) and np.array_equal(nv > 0, v > 0)
        assert np.array_equal(u32(nv[~act]), u32(v[~act]))
        v = nv


def ball(n=32, seed=7):
    """A jittered ball: the lattice of spacing 0.5 inside radius 6 round the centre, each point moved by up to 0.2 per axis."""
    r = np.arange(-6.0, 6.01, 0.5)
    p = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    p = p[(p ** 2).sum(axis=1) <= 36.0]
    return p + np.random.default_rng(seed).uniform(-0.2, 0.2, p.shape)


def test_tracking_brings_the_gradient_back_to_one():
    """The jittered ball at n = 32, (R, w, dx) = (2, 2, 1): mean | |grad| - 1 | over the active voxels with |val| < bg / 2 of the
    (1, 4) filter, tracked (N = 3, trim) against untracked.  The ordering is asserted; the figures are DESIGN f13's."""
    n, (R, w, dx) = 32, (2.0, 2.0, 1.0)
    pos = ball(n)
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    bg = sdf_ref.constants(R, w, dx)[3]
    raw = T.gradient_error(val, act, bg, dx)
    res = {}
    for W, K in ((1, 1), (1, 4), (2, 4)):
        plain = sdf_filter_ref.smooth(val, act, bg, W, K)
        vt, at = T.tracked(val, act, bg, dx, W, K, 0.0, 3, True)
        res[(W, K)] = (T.gradient_error(plain, act, bg, dx), T.gradient_error(vt, at, bg, dx))
        assert np.isfinite(vt).all()
    print("particles", len(pos), "raw", raw, res)
    assert len(pos) == 7153
    for k, (untracked, tracked) in res.items():
        assert tracked < untracked, (k, untracked, tracked)


def test_the_case_list_holds_what_the_gpu_tests_rely_on():
    """Over scenes x n x SETS x TRACKS: a case where the trim deactivates voxels and every leaf stays, one where some but not all
    leaves leave the list, one where the list becomes empty; and the two named ones."""
    kinds = {"stay": 0, "some": 0, "empty": 0}
    seen = {}
    for name in SCENES:
        for n in (16, 25):
            for R, w, dx in mesh_ref.SETS:
                _, val, act, bg, _ = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))
                l0 = leaves(val, act, bg)
                for case in T.TRACKS:
                    _, vt, at, _, _ = T.scene(name, n, R, w, dx, case)
                    l1, gone = leaves(vt, at, bg), int(act.sum() - at.sum())
                    seen[(name, n, R, w, dx) + case] = (l0, l1, gone)
                    if gone > 0:
                        kinds["stay" if l1 == l0 else "empty" if l1 == 0 else "some"] += 1
    assert all(v > 0 for v in kinds.values()), kinds
    assert seen[("one", 16, 1.5, 2.5, 1.0, 1, 1, 0.0, 3, 1)] == (8, 8, 42)
    assert seen[("hi", 25, 1.5, 2.5, 1.0, 1, 1, 0.0, 3, 1)] == (5, 4, 55)
    assert seen[("cloud", 25, 1.5, 2.5, 1.0, 1, 1, 0.0, 3, 1)] == (61, 60, 225)
    assert seen[("one", 16, 1.5, 2.5, 1.0, 4, 3, 0.0, 2, 1)] == (8, 0, 269)
    assert seen[("cloud", 25, 3.0, 1.0, 1.0, 1, 0, 0.6, 2, 1)][:2] == (61, 60)
