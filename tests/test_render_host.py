"""CPU: the host side of "liquid surface as an image" — fluid_sdf_render on leaf lists equals tests/render_ref.py (rgb bytes, depth
and normals as bit patterns, n_hit) on every scene tests/test_gpu_render.py uses, its refusals, fluid_write_png re-read through
Python's zlib, fluid_camera_look_at."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import render_ref as rr
import render_scenes as rs
import sdf_ref

SETS = rs.SETS
ERR_ARG = 1


def host(fs, n, val, act, bg, R, w, cam, what=7, shade=rs.SHADE):
    return fs.sdf_render(rs.leaf_grid(fs, n, val, act, bg, R, w), fs.camera(*cam), shade, bool(what & 1), bool(what & 2), bool(what & 4))


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name,n", [(name, 32) for name in ("one", "corner", "lo", "hi", "cloud")] + [("one", 16)])
def test_named_scenes(fs, name, n, R, w, dx):
    pos, val, act, bg = rs.named(name, n, R, w, dx)
    cam = rs.named_camera(name, n)
    ref = rs.reference((name, n, R, w, dx), val, bg, cam)
    assert 0.05 < ref["n_hit"] / (cam.width * cam.height) < 0.95, ref["n_hit"]
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref, note=name)


def test_every_what_and_the_default_shade(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    cam = rs.named_camera("cloud", n)
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    for what in range(1, 8):
        rs.same(host(fs, n, val, act, bg, R, w, cam, what), ref, what)
    white = rs.reference(("cloud", n, R, w, dx), val, bg, cam, ((1.0, 1.0, 1.0), (0, 0, 0)))
    rs.same(host(fs, n, val, act, bg, R, w, cam, 7, None), white)
    assert (ref["rgb"][..., 2] == 255).any() and not np.array_equal(white["rgb"], ref["rgb"])     # base 1.7 clamps


@pytest.mark.parametrize("name", ["corner", "cloud"])
def test_orthographic_rays_in_leaf_faces(fs, name):
    n, (R, w, dx) = 32, SETS[1]
    pos, val, act, bg = rs.named(name, n, R, w, dx)
    grid = rs.leaf_grid(fs, n, val, act, bg, R, w)
    hits = 0
    for o in rs.ORTHO:
        cam = rs.ortho(*o)
        ref = rs.reference((name, n, R, w, dx), val, bg, cam)
        hits += ref["n_hit"] > 0
        rs.same(fs.sdf_render(grid, fs.camera(*cam), rs.SHADE, True, True, True), ref, note=o)
    assert hits >= 6 and (name == "cloud" or hits < len(rs.ORTHO))            # every axis and sign hits; the lone particle is also missed


def test_eye_in_the_liquid_and_eye_in_the_air(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    cam = rs.pinhole(target=(0.0, 0.0, 0.0), eye=tuple(pos[0]))
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert (ref["k_hit"] == 0).all() and (ref["depth"] == 0).all()           # t = t_0 = t_near
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)
    eye = rs.air_eye(val, n, bg)
    cells = sdf_ref.base_cell(pos)
    assert (np.array(eye) > cells.min(axis=0) - 4).all() and (np.array(eye) < cells.max(axis=0) + 4).all()   # inside the range's box
    cam = rs.pinhole(target=tuple(pos[1]), eye=eye, fov=90.0)
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert (ref["k_hit"] != 0).all() and (ref["k_hit"] > 0).sum() > 100 and (ref["k_hit"] < 0).sum() > 0
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)


def test_all_misses(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    cam = rs.pinhole(target=(-60.0, 20.0, -80.0))
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert ref["n_hit"] == 0
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)
    # no leaf at all: NULL arrays behind an empty list
    empty = fs.SdfGrid(n, np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 512), bool), bg, R, w)
    rs.same(fs.sdf_render(empty, fs.camera(*rs.named_camera("cloud", n)), rs.SHADE, True, True, True), ref)


def test_huge_steps_run_far_out_of_bounds(fs):
    """4 x 4, step 1e3, 65536 samples: t reaches 6.5e7, every sample but the first few is out of bounds by the rule, nothing is
    converted to int there."""
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    cam = rs.pinhole(width=4, height=4, step=1e3, n_steps=65536)
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert ref["n_hit"] == 0
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)
    cam = rs.pinhole(width=4, height=4, step=1e3, n_steps=65536, eye=tuple(pos[0]))   # k = 0 in the liquid, then gone
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert ref["n_hit"] == 16
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)


@pytest.mark.parametrize("filt", [(1, 1, 0.0), (1, 4, -0.5)])
def test_filtered_cloud(fs, filt):
    n, (R, w, dx) = 32, SETS[1]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx, filt)
    cam = rs.named_camera("cloud", n)
    ref = rs.reference(("cloud", n, R, w, dx, filt), val, bg, cam)
    plain = rs.reference(("cloud", n, R, w, dx), rs.named("cloud", n, R, w, dx)[1], bg, cam)
    assert ref["n_hit"] > 200 and not np.array_equal(ref["rgb"], plain["rgb"])
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)
    # the host filter's values are the reference filter's
    g = fs.sdf_filter(rs.leaf_grid(fs, n, *rs.named("cloud", n, R, w, dx)[1:], R, w), *filt)
    rs.same(fs.sdf_render(g, fs.camera(*cam), rs.SHADE, True, True, True), ref)


def test_filtered_surface_reaches_the_fifth_ring(fs):
    """The one-particle scene of tests/test_gpu_render.py whose filtered surface has negative values four cells from the base cell."""
    n, (R, w, dx), filt = 32, (3.0, 1.0, 1.0), (1, 0, -0.9)
    pos = np.array([[-4.49, -4.49, -4.49]])
    val, act, bg = rs.level_set(pos, n, R, w, dx, filt)
    cam = rs.pinhole(tuple(pos[0]), 12.0, eye=(-40.0, -30.0, -35.0))
    ref = rs.reference(("fifth", filt), val, bg, cam)
    assert 0.05 < (ref["k_hit"] >= 0).mean() < 0.95 and (np.floor(rs.hit_points(cam, ref)).min(axis=0) == -9).all()
    rs.same(host(fs, n, val, act, bg, R, w, cam), ref)


def test_refusals(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("one", n, R, w, dx)
    grid = rs.leaf_grid(fs, n, val, act, bg, R, w)
    c, _keep = grid._c()
    good = rs.named_camera("one", n)
    px = good.width * good.height
    rgb, depth, nrm = np.full(3 * px, 7, np.uint8), np.full(px, 7, np.float32), np.full(3 * px, 7, np.float32)
    hit = C.c_int64(-5)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(cam=None, shade=None, what=7, grid_c=c, arrays=(rgb, depth, nrm)):
        cam = fs.camera(*good) if cam is None else cam
        return fs.lib.fluid_sdf_render(C.byref(grid_c), C.byref(cam), None if shade is None else C.byref(shade), what,
                                       *[None if a is None else ptr(a) for a in arrays], C.byref(hit))

    def cam_with(**kw):
        d = good._asdict()
        d.update(kw)
        cam = fs.Camera()
        for k, v in d.items():
            setattr(cam, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
        return cam

    bad_cams = [cam_with(width=0), cam_with(width=8193), cam_with(height=0), cam_with(height=8193), cam_with(width=8192, height=4096),
                cam_with(n_steps=0), cam_with(n_steps=65537), cam_with(step=0.0), cam_with(step=-0.5), cam_with(step=float("inf")),
                cam_with(step=float("nan")), cam_with(t_near=-1.0), cam_with(t_near=float("inf")), cam_with(eye=(0.0, float("nan"), 0.0)),
                cam_with(dir00=(float("inf"), 0.0, 0.0)), cam_with(du=(0.0, 0.0, float("nan"))), cam_with(dv=(0.0, float("-inf"), 0.0))]
    for i, cam in enumerate(bad_cams):
        assert call(cam=cam) == ERR_ARG, i
    f3, b3 = C.c_float * 3, C.c_uint8 * 3
    assert call(shade=fs.Shade(f3(1, float("nan"), 1), b3(0, 0, 0), 0)) == ERR_ARG
    assert call(shade=fs.Shade(f3(1, 1, 1), b3(0, 0, 0), 1)) == ERR_ARG
    for what in (0, 8, 15, 0x80000001):
        assert call(what=what) == ERR_ARG, what
    assert call(arrays=(None, depth, nrm)) == ERR_ARG and call(arrays=(rgb, None, nrm)) == ERR_ARG and call(arrays=(rgb, depth, None)) == ERR_ARG
    assert call(what=2, arrays=(None, depth, None)) == 0 and hit.value > 0     # a part that is not asked for needs no array
    depth[:] = 7
    hit.value = -5
    org = grid.origin.copy()
    org[0, 0] += 1                                                              # off the 8-grid: what fluid_sdf_to_dense refuses
    bad = fs.SdfGrid(n, org, grid.values, grid.active, bg, R, w)
    cb, _keep2 = bad._c()
    assert call(grid_c=cb) == ERR_ARG
    assert fs.lib.fluid_sdf_render(C.byref(c), None, None, 7, ptr(rgb), ptr(depth), ptr(nrm), C.byref(hit)) == ERR_ARG
    assert fs.lib.fluid_sdf_render(None, C.byref(fs.camera(*good)), None, 7, ptr(rgb), ptr(depth), ptr(nrm), C.byref(hit)) == ERR_ARG
    # nothing was written by any refused call
    assert (rgb == 7).all() and (depth == 7).all() and (nrm == 7).all() and hit.value == -5
    assert call(cam=cam_with(width=4096, height=4096, n_steps=1), what=2, arrays=(None, np.empty(1 << 24, np.float32), None)) == 0   # the largest image
    with pytest.raises(fs.FluidError):
        fs.sdf_render(bad, fs.camera(*good))


def read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data)
        chunks.append((kind, data))
        at += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_png_round_trip(fs, tmp_path):
    rng = np.random.default_rng(1)
    for shape in ((1, 1, 3), (32, 48, 3), (5, 7, 3), (360, 640, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        fs.write_png(tmp_path / "a.png", img)
        assert np.array_equal(read_png(tmp_path / "a.png"), img), shape
    img = np.zeros((2, 2, 3), np.uint8)
    assert fs.lib.fluid_write_png(None, 2, 2, img.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert fs.lib.fluid_write_png(str(tmp_path / "b.png").encode(), 2, 2, None) == ERR_ARG
    for w, h in ((0, 2), (2, 0), (8193, 2), (2, 8193)):
        assert fs.lib.fluid_write_png(str(tmp_path / "b.png").encode(), w, h, img.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert fs.lib.fluid_write_png(str(tmp_path / "no" / "such" / "dir.png").encode(), 2, 2, img.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert not (tmp_path / "b.png").exists()
    with pytest.raises(fs.FluidError):
        fs.write_png(tmp_path / "no" / "b.png", img)


def test_camera_look_at(fs, tmp_path):
    n = 32
    eye, target, up = (-30.0, 10.0, -40.0), (1.0, -2.0, 0.5), (0.0, 1.0, 0.0)
    c = fs.camera_look_at(n, eye, target, up, 40.0, 48, 32, 0.5)
    ref = rr.pinhole(eye, target, up, 40.0, 48, 32, 0.5, 1)
    for k in ("eye", "dir00", "du", "dv"):
        got, exp = np.array(list(getattr(c, k)), np.float64), np.array(getattr(ref, k))
        assert np.abs(got - exp).max() <= 1e-6 * np.abs(exp).max(), k
    assert (c.width, c.height, c.t_near, c.step) == (48, 32, 0.0, 0.5)
    # the march just passes the farthest corner of [lo - 1, hi + 1]^3
    far = np.sqrt(sum(max(abs(e + 17), abs(e - 16)) ** 2 for e in eye))
    assert far / 0.5 <= c.n_steps <= far / 0.5 + 4
    assert fs.camera_look_at(4096, (9000.0, 0.0, 0.0), step=0.01).n_steps == 65536
    # the centre ray points at the target; rows run down, columns to the right of the view
    fw = np.array(target) - np.array(eye)
    fw /= np.linalg.norm(fw)
    mid = np.array(list(c.dir00)) + 24 * np.array(list(c.du)) + 16 * np.array(list(c.dv))
    assert np.abs(mid / np.linalg.norm(mid) - fw).max() < 1e-6
    assert np.array(list(c.dv))[1] < 0 and abs(np.dot(list(c.du), list(c.dv))) < 1e-9 and abs(np.dot(list(c.du), fw)) < 1e-7
    assert np.isclose(np.linalg.norm(list(c.du)), np.linalg.norm(list(c.dv))) and np.isclose(np.linalg.norm(list(c.dv)) * 32, 2 * np.tan(np.radians(20.0)))
    # rendering through it shows the scene
    R, w, dx = SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    cam = fs.camera_look_at(n, (-30.0, 10.0, -40.0), width=48, height=32)
    out = fs.sdf_render(rs.leaf_grid(fs, n, val, act, bg, R, w), cam, depth=True)
    assert 0.15 < out["n_hit"] / (48 * 32) < 0.25 and out["rgb"][16, 24].min() > 0 and (out["rgb"][0, 0] == 0).all()
    fs.write_png(tmp_path / "cloud.png", out["rgb"])
    assert np.array_equal(read_png(tmp_path / "cloud.png"), out["rgb"])
    d3 = lambda v: (C.c_double * 3)(*v)   # noqa: E731
    out_c = fs.Camera()
    bad = [dict(n=0), dict(eye=target), dict(up=tuple(np.array(target) - np.array(eye))), dict(fov=0.0), dict(fov=180.0), dict(width=0), dict(height=8193),
           dict(width=8192, height=4096), dict(step=0.0), dict(step=float("nan")), dict(eye=(float("nan"), 0.0, 0.0)), dict(up=(0.0, 0.0, 0.0))]
    for kw in bad:
        a = dict(n=n, eye=eye, target=target, up=up, fov=40.0, width=48, height=32, step=0.5)
        a.update(kw)
        assert fs.lib.fluid_camera_look_at(a["n"], d3(a["eye"]), d3(a["target"]), d3(a["up"]), a["fov"], a["width"], a["height"], a["step"], C.byref(out_c)) == ERR_ARG, kw
    with pytest.raises(fs.FluidError):
        fs.camera_look_at(n, eye, eye)
