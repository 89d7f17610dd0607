"""CPU: the numpy restatement of "liquid surface as an image" (tests/render_ref.py) against things that are not the code under test —
the lemma that lets an implementation skip empty space, the geometry of one sphere, the behaviour under a halved step."""
import numpy as np
import pytest

import render_ref as rr
import render_scenes as rs

F = np.float32
CENTRE = np.array([0.3, -0.2, 0.41])


def test_lerp_of_non_negative_ends_is_non_negative():
    """For a, b >= 0 and t in [0, 1], a + t * (b - a) >= 0 in float32, each operation rounded: 2 M triples — magnitudes over the whole
    exponent range, denormals, zeros, equal ends, t = 0, 1, 1 - ulp, ulp —, none negative (and none -0).  This is what allows a cell
    whose corners are all >= 0 to be skipped: its trilinear value is seven such lerps."""
    rng = np.random.default_rng(7)
    m = 2_000_000
    bits = lambda: rng.integers(0, 0x7f800000, m, dtype=np.uint32).view(F)      # noqa: E731  every finite non-negative float
    a, b = bits(), bits()
    a[:1000], b[1000:2000] = 0, 0
    a[2000:200_000] = rng.integers(0, 0x00800000, 198_000, dtype=np.uint32).view(F)              # denormals
    b[100_000:300_000] = rng.integers(0, 0x00800000, 200_000, dtype=np.uint32).view(F)
    near = slice(300_000, 600_000)                                                               # ends a few ulps apart
    b[near] = (a[near].view(np.uint32) + rng.integers(0, 4, 300_000, dtype=np.uint32)).view(F)
    b[near] = np.where(np.isfinite(b[near]), b[near], a[near])
    t = rng.uniform(0, 1, m).astype(F)
    one_less = np.nextafter(F(1), F(0))
    t[::7], t[1::7], t[2::7], t[3::7] = one_less, F(1), F(0), np.nextafter(F(0), F(1))
    assert (t >= 0).all() and (t <= 1).all() and (t == one_less).sum() > 100_000
    with np.errstate(over="ignore", under="ignore"):
        for x, y in ((a, b), (b, a)):
            r = rr._lerp(x, y, t)
            assert r.dtype == F and not (r < 0).any() and not np.signbit(r).any()
    # and the seven lerps of a cell with corners >= 0
    v = rng.integers(0, 0x7f000000, (200_000, 8), dtype=np.uint32).view(F)
    f = np.stack([t[:200_000], t[200_000:400_000], t[400_000:600_000]], axis=1)
    with np.errstate(over="ignore", under="ignore"):
        assert not (rr._trilinear(v, f) < 0).any()


def sphere(R, w, step):
    """(reference image, analytic depth (nan: the ray misses the sphere), unit rays, camera) of one sphere at CENTRE, n = 32."""
    n, dx = 32, 1.0
    val, _, bg = rs.level_set(CENTRE[None, :], n, R, w, dx)
    cam = rs.pinhole(tuple(CENTRE), 8.0, step=step, n_steps=int(100 / step))
    out = rr.render(val, bg, cam)
    eye = np.array(cam.eye, np.float64)
    jj, ii = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    D = np.array(cam.dir00) + (ii[..., None] + 0.5) * np.array(cam.du) + (jj[..., None] + 0.5) * np.array(cam.dv)
    d = D / np.linalg.norm(D, axis=-1, keepdims=True)
    oc = eye - CENTRE
    b = (d * oc).sum(-1)
    disc = b * b - ((oc * oc).sum() - R * R)
    with np.errstate(invalid="ignore"):
        ta = -b - np.sqrt(np.where(disc > 0, disc, np.nan))
    return out, ta, d, eye


@pytest.mark.parametrize("R,w,max_err,min_dot", [(2.0, 2.0, 0.6249, 0.94873), (3.0, 1.0, 0.6181, 0.97707)])
def test_one_sphere_against_the_analytic_intersection(R, w, max_err, min_dot):
    """The reference against geometry, step 0.25, a 48 x 32 pinhole of 8 degrees aimed at the sphere.  Measured: (R, w) = (2, 2):
    largest |depth - analytic| 0.6249 voxels, smallest n . r 0.94873; (3, 1): 0.6181 and 0.97707 — both at grazing rays, where the
    trilinear surface of a sphere of two or three voxels is at its worst.  Asserted: twice the error, and twice the deficit from 1
    (the measured value uses half of what is allowed)."""
    out, ta, d, eye = sphere(R, w, 0.25)
    hit = out["k_hit"] >= 0
    assert 200 < hit.sum() == out["n_hit"] and (out["k_hit"][hit] > 0).all()
    assert (hit & np.isnan(ta)).sum() <= 0.02 * hit.sum()                  # the silhouettes agree but for a rim of pixels
    assert (np.isfinite(ta) & ~hit).sum() < 0.15 * np.isfinite(ta).sum()
    both = hit & np.isfinite(ta)
    err = np.abs(out["depth"].astype(np.float64) - ta)[both].max()
    r = eye + out["depth"][..., None].astype(np.float64) * d - CENTRE
    with np.errstate(invalid="ignore"):
        dot = ((out["normals"].astype(np.float64) * r).sum(-1) / np.linalg.norm(r, axis=-1))[hit].min()
    print(f"(R, w) = {(R, w)}: max depth error {err:.4f}, min n.r {dot:.5f}")
    assert err <= 2 * max_err and dot >= 1 - 2 * (1 - min_dot)
    ln = np.linalg.norm(out["normals"].astype(np.float64), axis=-1)
    assert np.allclose(ln[hit], 1.0, atol=1e-6) and (out["normals"][~hit] == 0).all() and np.isposinf(out["depth"][~hit]).all()
    # the shade is |n . d| through the clamp: white base, black background
    s = np.abs((out["normals"].astype(np.float64) * d).sum(-1))
    assert np.abs(out["rgb"][..., 0].astype(np.float64) - 255 * s)[hit].max() < 0.51 and (out["rgb"][~hit] == 0).all()


def test_halving_the_step_moves_no_depth_by_more_than_one_old_step():
    a, b = sphere(2.0, 2.0, 0.25)[0], sphere(2.0, 2.0, 0.125)[0]
    both = (a["k_hit"] >= 0) & (b["k_hit"] >= 0)
    assert both.sum() > 200 and ((a["k_hit"] >= 0) & ~both).sum() == 0     # a finer march loses no hit
    assert np.abs(a["depth"][both].astype(np.float64) - b["depth"][both]).max() <= 0.25


def test_looking_away_misses_everywhere():
    pos, val, act, bg = rs.named("cloud", 32, *rs.SETS[0])
    out = rr.render(val, bg, rs.pinhole(target=(-60.0, 20.0, -80.0)), *rs.SHADE)
    assert out["n_hit"] == 0 and (out["k_hit"] == -1).all() and np.isposinf(out["depth"]).all() and (out["normals"] == 0).all()
    assert (out["rgb"] == np.array(rs.SHADE[1], np.uint8)).all()


def test_a_degenerate_direction_is_a_miss():
    pos, val, act, bg = rs.named("cloud", 32, *rs.SETS[0])
    out = rr.render(val, bg, rr.camera(pos[0], (0, 0, 0), (0, 0, 0), (0, 0, 0), 2, 2, 0.0, 0.5, 4))   # in the liquid, no direction
    assert out["n_hit"] == 0 and np.isposinf(out["depth"]).all()
