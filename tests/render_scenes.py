"""The scenes and cameras the render tests share (tests/test_render_host.py on the CPU, tests/test_gpu_render.py on the device) — test
infrastructure, numpy only.  A case is (particles, n, (R, w, dx), filter or None, camera); its reference (tests/render_ref.py on the
dense level set of tests/sdf_ref.py, filtered through tests/sdf_filter_ref.py) is computed once per process and never modified.
Images are at most 48 x 32 and a ray has at most 200 samples, except where a case is about the sample count."""
import numpy as np

import mesh_ref
import render_ref as rr
import sdf_filter_ref
import sdf_ref
from sdf_testlib import u32

SETS = mesh_ref.SETS
EYE = (-30.0, 10.0, -40.0)                                      # outside every grid used here
SHADE = ((0.9, 0.5, 1.7), (3, 200, 77))                         # base (one channel clamps), background


def pinhole(target=(0.0, 0.0, 0.0), fov=40.0, eye=EYE, width=48, height=32, step=0.5, n_steps=200):
    return rr.pinhole(eye, target, (0.0, 1.0, 0.0), fov, width, height, step, n_steps)


def named_camera(name, n):
    """The 48 x 32 pinhole from EYE with step 0.5: at the cloud with 40 degrees; at a scene of one or two particles aimed at the
    first of them, with the field of view in which a sphere of one voxel at that distance is 7.5 pixels in radius: spheres of 1
    to 3 voxels then fill between a twentieth and most of the image."""
    if name == "cloud":
        return pinhole()
    p = mesh_ref.positions(name, n)[0]
    return pinhole(tuple(p), float(np.degrees(32.0 / (7.5 * np.linalg.norm(p - np.array(EYE))))))


def ortho(axis, sign, u, v, n=32):
    """Every pixel of a 2 x 2 image is the ray from a point with the integer coordinates (u, v) on the two other axes, 8 outside the
    grid, along +-axis: the direction has two exact zeros, samples fall on voxel planes, and (u, v) multiples of 8 put the ray inside
    leaf faces."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    eye, d = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    b1, b2 = [x for x in range(3) if x != axis]
    eye[axis] = float(lo - 8) if sign > 0 else float(hi + 9)
    eye[b1], eye[b2] = float(u), float(v)
    d[axis] = float(sign)
    return rr.camera(eye, d, (0, 0, 0), (0, 0, 0), 2, 2, 0.0, 0.5, 2 * (n + 16))


ORTHO = [(axis, sign, u, v) for axis in range(3) for sign in (1, -1) for (u, v) in ((0, 0), (-8, 0), (0, 8), (8, -8))]

_cache = {}


def level_set(pos, n, R, w, dx, filt=None):
    """(val, act, bg) of a particle set, filtered if asked for."""
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    bg = sdf_ref.constants(R, w, dx)[3]
    if filt is not None:
        val = sdf_filter_ref.smooth(val, act, bg, *filt)
    return val, act, bg


def named(name, n, R, w, dx, filt=None):
    """(positions, val, act, bg) of a named scene of tests/mesh_ref.py; cached."""
    key = ("ls", name, n, R, w, dx, filt)
    if key not in _cache:
        pos = mesh_ref.positions(name, n)
        val, act, bg = level_set(pos, n, R, w, dx, filt)
        for a in (val, act):
            a.setflags(write=False)
        _cache[key] = (pos, val, act, bg)
    return _cache[key]


def reference(key, val, bg, cam, shade=SHADE):
    """render_ref.render, cached under key."""
    key = ("img", key, cam, shade)
    if key not in _cache:
        out = rr.render(val, bg, cam, *shade)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def leaf_grid(fs, n, val, act, bg, R, w):
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    return fs.SdfGrid(n, org, v, a, bg, R, w)


def same(got, ref, what=7, note=""):
    """The parts `what` names equal the reference (floats as bit patterns), the others are None; n_hit is the reference's."""
    assert got["n_hit"] == ref["n_hit"], (note, got["n_hit"], ref["n_hit"])
    for bit, key in ((1, "rgb"), (2, "depth"), (4, "normals")):
        if not (what & bit):
            assert got[key] is None, (note, what, key)
        elif key == "rgb":
            assert got[key].dtype == np.uint8 and got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), (note, what, key)
        else:
            assert got[key].dtype == np.float32 and got[key].shape == ref[key].shape and np.array_equal(u32(got[key]), u32(ref[key])), (note, what, key)


def air_eye(val, n, bg):
    """A quarter into the cell of the voxel closest to the origin (ties: the first in array order) whose 3^3 neighbourhood is all
    > 0: an eye in the air."""
    lo = sdf_ref.geometry(n)[0]
    far = val > np.float32(0)
    ok = np.ones((n - 2,) * 3, bool)
    for d in np.ndindex(3, 3, 3):
        ok &= far[d[0]:d[0] + n - 2, d[1]:d[1] + n - 2, d[2]:d[2] + n - 2]
    c = np.argwhere(ok) + 1 + lo
    return tuple(float(x) + 0.25 for x in c[np.argmin((c.astype(np.int64) ** 2).sum(axis=1))])


def hit_points(cam, ref):
    """(hits, 3) float64: eye + depth * d of the hit pixels, to float64 accuracy (for assertions about where a case hits)."""
    jj, ii = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    D = np.array(cam.dir00) + (ii[..., None] + 0.5) * np.array(cam.du) + (jj[..., None] + 0.5) * np.array(cam.dv)
    d = D / np.linalg.norm(D, axis=-1, keepdims=True)
    hit = ref["k_hit"] >= 0
    return np.array(cam.eye) + ref["depth"][hit][:, None].astype(np.float64) * d[hit]
