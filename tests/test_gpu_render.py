"""GPU (-m gpu): images of the liquid surface (fluid_render_snapshot / fluid_render_wait; k_render_neg, k_render_occ, k_render_march).
In every comparison the device result equals tests/render_ref.py — rgb bytes exactly, depth and normals as bit patterns, the hit
count —, and where a downloaded list is at hand fluid_sdf_render gives the same bytes again.  The reference evaluates every sample
of every ray; the kernel skips empty leaves and clips to the range, so every case here is also a test of what it may skip.  Each
situation a case is named after is asserted from the reference before the device is asked."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import render_ref as rr
import render_scenes as rs
import sdf_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = rs.SETS
ERR_ARG, ERR_STATE = 1, 3


def pad16(x):
    return (x + 15) & ~15


def bytes_to_host(cam, what):
    px = cam.width * cam.height
    return 16 + (pad16(3 * px) if what & 1 else 0) + (4 * px if what & 2 else 0) + (12 * px if what & 4 else 0)


def shoot(fs, sim, R, w, cam, what=7, filt=None, shade=rs.SHADE):
    sim.render_snapshot(R, w, fs.camera(*cam), smooth=filt, shade=shade, rgb=bool(what & 1), depth=bool(what & 2), normals=bool(what & 4))
    assert sim.render_stats()["bytes_to_host"] == bytes_to_host(cam, what) and sim.render_stats()["pixels"] == cam.width * cam.height
    out = sim.render_wait()
    assert sim.render_stats()["hits"] == out["n_hit"]
    return out


def check(fs, sim, ref, R, w, cam, filt=None, what_all=range(1, 8), note=""):
    for what in what_all:
        rs.same(shoot(fs, sim, R, w, cam, what, filt), ref, what, (note, what))


CASES = [(name, 32) for name in ("one", "corner", "lo", "hi", "cloud")] + [("one", 16)]


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name,n", CASES)
def test_every_scene_and_every_what(fs, name, n, R, w, dx):
    pos, val, act, bg = rs.named(name, n, R, w, dx)
    cam = rs.named_camera(name, n)
    ref = rs.reference((name, n, R, w, dx), val, bg, cam)
    assert 0.05 < ref["n_hit"] / (cam.width * cam.height) < 0.95
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    check(fs, sim, ref, R, w, cam, note=f"{name} {n} {(R, w, dx)}")
    if name == "corner":                                                    # eight leaves meet at the particle: hit cells read them all
        sim.sdf_snapshot(R, w)
        assert sim.sdf_wait().n_leaves == 8
    sim.close()


@pytest.mark.parametrize("name", ["corner", "cloud"])
def test_orthographic_rays_in_leaf_faces(fs, name):
    """Rays along +-x, +-y, +-z from eyes on multiples of 8: the direction has two exact zeros (no exit plane on those axes), the
    samples lie in leaf faces and on voxel planes (f = 0, cells and leaves change exactly at a sample)."""
    n, (R, w, dx) = 32, SETS[1]
    pos, val, act, bg = rs.named(name, n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    hits = 0
    for o in rs.ORTHO:
        cam = rs.ortho(*o)
        assert sorted(np.abs(cam.dir00)) == [0.0, 0.0, 1.0] and all(float(e) % 8 == 0 for e in cam.eye)
        ref = rs.reference((name, n, R, w, dx), val, bg, cam)
        hits += ref["n_hit"] > 0
        rs.same(shoot(fs, sim, R, w, cam), ref, note=(name, o))
    assert hits >= 6 and (name == "cloud" or hits < len(rs.ORTHO))
    sim.close()


def test_eye_in_the_liquid_and_eye_in_the_air(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    cam = rs.pinhole(target=(0.0, 0.0, 0.0), eye=tuple(pos[0]))
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert (ref["k_hit"] == 0).all() and (ref["depth"] == 0).all()
    check(fs, sim, ref, R, w, cam, what_all=(7, 2), note="eye in the liquid")
    eye = rs.air_eye(val, n, bg)
    cells = sdf_ref.base_cell(pos)
    assert (np.array(eye) > cells.min(axis=0) - 4).all() and (np.array(eye) < cells.max(axis=0) + 4).all()   # inside the range's box
    cam = rs.pinhole(target=tuple(pos[1]), eye=eye, fov=90.0)
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    assert (ref["k_hit"] != 0).all() and (ref["k_hit"] > 0).sum() > 100 and (ref["k_hit"] < 0).sum() > 0
    check(fs, sim, ref, R, w, cam, what_all=(7,), note="eye in the air")
    sim.close()


def test_all_misses_and_no_particle(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    away = rs.pinhole(target=(-60.0, 20.0, -80.0))
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, away)
    assert ref["n_hit"] == 0
    sim = fs.FluidSim(n=n, dx=dx)
    cam = rs.named_camera("cloud", n)
    for what in range(1, 8):                                                # no particle at all: the record is still there
        out = shoot(fs, sim, R, w, cam, what)
        rs.same(out, ref, what, ("no particle", what))
    sim.upload_particles(pos)
    check(fs, sim, ref, R, w, away, note="looking away")
    # particles that do not count (base cell off the grid) are no particles
    sim.upload_particles(np.array([[40.0, 0.0, 0.0]]))
    rs.same(shoot(fs, sim, R, w, cam), ref, note="off the grid")
    sim.close()


def test_huge_steps_run_far_out_of_bounds(fs):
    n, (R, w, dx) = 32, SETS[0]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    for eye, hits in ((rs.EYE, 0), (tuple(pos[0]), 16)):
        cam = rs.pinhole(width=4, height=4, step=1e3, n_steps=65536, eye=eye)
        ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
        assert ref["n_hit"] == hits
        rs.same(shoot(fs, sim, R, w, cam), ref, note=eye)
    sim.close()


@pytest.mark.parametrize("filt", [(1, 1, 0.0), (1, 4, -0.5)])
def test_filtered_cloud(fs, filt):
    n, (R, w, dx) = 32, SETS[1]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx, filt)
    cam = rs.named_camera("cloud", n)
    ref = rs.reference(("cloud", n, R, w, dx, filt), val, bg, cam)
    plain = rs.reference(("cloud", n, R, w, dx), rs.named("cloud", n, R, w, dx)[1], bg, cam)
    assert ref["n_hit"] > 200 and not np.array_equal(ref["rgb"], plain["rgb"])
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    check(fs, sim, ref, R, w, cam, filt, note=f"cloud {filt}")
    check(fs, sim, plain, R, w, cam, what_all=(7,), note="unfiltered after filtered")
    sim.close()


def test_filtered_surface_reaches_the_fifth_ring(fs):
    """One particle at (-4.49)^3, n = 32, (R, w) = (3, 1), offset -0.9 (tests/test_gpu_mesh_normals.py): negative values four
    cells from the base cell, hit cells in the leaf at -16 — inside the range only because it is the box dilated by 5."""
    n, (R, w, dx), filt = 32, (3.0, 1.0, 1.0), (1, 0, -0.9)
    pos = np.array([[-4.49, -4.49, -4.49]])
    val, act, bg = rs.level_set(pos, n, R, w, dx, filt)
    cam = rs.pinhole(tuple(pos[0]), 12.0, eye=(-40.0, -30.0, -35.0))
    ref = rs.reference(("fifth", filt), val, bg, cam)
    assert 0.05 < (ref["k_hit"] >= 0).mean() < 0.95
    assert ((np.argwhere(val < 0) - 16).min(axis=0) == -8).all()           # a cell with such a corner has its min corner at -9 = base - 5
    assert (np.floor(rs.hit_points(cam, ref)).min(axis=0) == -9).all()     # and such cells are hit
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos)
    check(fs, sim, ref, R, w, cam, filt, note="dilate 5")
    sim.close()


def test_cloud_and_stale_scratch(fs):
    """The cloud, then one particle far from where the cloud's listed leaves were, then the cloud again, render snapshots only:
    the search leaves the unreached leaves of the new range at once, and the cloud's values in the scratch must not be read."""
    n, (R, w, dx) = 32, SETS[3]
    pos, val, act, bg = rs.named("cloud", n, R, w, dx)
    cam = rs.named_camera("cloud", n)
    ref = rs.reference(("cloud", n, R, w, dx), val, bg, cam)
    sim = fs.FluidSim(n=n, dx=dx)
    for p in (None, [[13.3, 13.2, -12.6]], None, [[13.3, 13.2, -12.6], [-13.4, -12.7, 13.1]], None):
        if p is None:
            sim.upload_particles(pos)
            r = ref
        else:
            far = np.array(p)
            sim.upload_particles(far)
            fv = rs.level_set(far, n, R, w, dx)[0]
            r = rr.render(fv, bg, cam, *rs.SHADE)
            assert 0 < r["n_hit"] < 40                                      # a small disc (or two) where the cloud was not
        for what in (7, 1):
            rs.same(shoot(fs, sim, R, w, cam, what), r, what, p)
    sim.close()


def test_after_steps_against_the_reference_and_the_host_function(fs):
    """The drop scene uploaded in a random order, 3 steps: the image is the reference's of the downloaded particles, and
    fluid_sdf_render on the downloaded level-set list gives the same bytes, raw and filtered."""
    n, (R, w, dx) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 4, seed=0)
    pos = pos[np.random.default_rng(9).permutation(len(pos))]
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    for _ in range(3):
        sim.step()
    p, _ = sim.download_particles()
    cam = rs.pinhole(eye=(-30.0, 25.0, -40.0))
    for filt in (None, (1, 1, -0.25)):
        val, act, bg = rs.level_set(p, n, R, w, dx, filt)
        ref = rr.render(val, bg, cam, *rs.SHADE)
        assert 0.1 < ref["n_hit"] / (48 * 32) < 0.9
        check(fs, sim, ref, R, w, cam, filt, what_all=(7, 1, 6), note=f"after 3 steps {filt}")
        sim.sdf_snapshot(R, w, smooth=filt)
        rs.same(fs.sdf_render(sim.sdf_wait(), fs.camera(*cam), rs.SHADE, True, True, True), ref, note=filt)
    sim.close()


def test_blocks_through_the_host_function_equal_one_gpu(fs):
    """2 x 2 x 2 blocks on one GPU: the ranks' lists merged and rendered on the host give the one-GPU snapshot of the same
    particles, byte for byte."""
    fd = fs.load_dist()
    n, dims, (R, w, dx) = 32, (2, 2, 2), SETS[0]
    rng = np.random.default_rng(32)
    ax = np.arange(-3, 3)
    c = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = np.repeat(c, 2, axis=0) + rng.uniform(-0.49, 0.49, (2 * len(c), 3))      # a block that straddles every cut
    grp = fd.LocalGroup(8)
    sims = [None] * 8

    def run(r):
        sims[r] = sim = fd.DistFluidSim(n, dims, fd.uniform_cuts(n, dims), grp.comms[r])
        sim.upload_global(pos)
        sim.sdf_snapshot(R, w)
        return sim.sdf_wait()

    try:
        parts = grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    merged = fs.merge_sdf_grids(parts)
    assert all(p.n_leaves > 0 for p in parts) and sum(p.n_leaves for p in parts) > merged.n_leaves
    cam = rs.pinhole(fov=25.0)
    one = fs.FluidSim(n=n)
    one.upload_particles(pos)
    for filt in (None, (1, 2, -0.25)):
        g = merged if filt is None else fs.sdf_filter(merged, *filt)
        host = fs.sdf_render(g, fs.camera(*cam), rs.SHADE, True, True, True)
        assert 0.1 < host["n_hit"] / (48 * 32) < 0.9
        rs.same(shoot(fs, one, R, w, cam, 7, filt), host, note=filt)
    one.close()


def test_slots_lifetimes_stats_and_refusals(fs):
    n, (R, w, dx) = 32, SETS[0]
    sim = fs.FluidSim(n=n)
    h = sim._h
    prm = fs.SdfParams(R, w)
    good = rs.named_camera("cloud", n)
    cam = fs.camera(*good)
    img = fs.ImageC()
    snap = lambda c=cam, what=7, p=prm, f=None, sh=None, hh=h: fs.lib.fluid_render_snapshot(   # noqa: E731
        hh, None if p is None else C.byref(p), None if f is None else C.byref(f), None if c is None else C.byref(c),
        None if sh is None else C.byref(sh), what)
    assert fs.lib.fluid_render_wait(h, C.byref(img)) == ERR_STATE                   # nothing outstanding
    assert "no render snapshot" in fs.lib.fluid_last_error().decode()
    assert sim.render_stats() == {"pixels": 0, "hits": 0, "bytes_to_host": 0}

    def cam_with(**kw):
        d = good._asdict()
        d.update(kw)
        c = fs.Camera()
        for k, v in d.items():
            setattr(c, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
        return c

    # every limit of the definition
    bad_cams = [cam_with(width=0), cam_with(width=8193), cam_with(height=0), cam_with(height=8193), cam_with(width=8192, height=4096),
                cam_with(n_steps=0), cam_with(n_steps=65537), cam_with(step=0.0), cam_with(step=-0.5), cam_with(step=float("inf")),
                cam_with(step=float("nan")), cam_with(t_near=-1.0), cam_with(t_near=float("inf")), cam_with(eye=(0.0, float("nan"), 0.0)),
                cam_with(dir00=(float("inf"), 0.0, 0.0)), cam_with(du=(0.0, 0.0, float("nan"))), cam_with(dv=(0.0, float("-inf"), 0.0))]
    for i, c in enumerate(bad_cams):
        assert snap(c=c) == ERR_ARG, i
    f3, b3 = C.c_float * 3, C.c_uint8 * 3
    assert snap(sh=fs.Shade(f3(1, float("inf"), 1), b3(0, 0, 0), 0)) == ERR_ARG
    assert snap(sh=fs.Shade(f3(1, 1, 1), b3(0, 0, 0), 1)) == ERR_ARG
    for what in (0, 8, 15, 0x80000001):
        assert snap(what=what) == ERR_ARG, what
    assert "what" in fs.lib.fluid_last_error().decode()
    assert snap(c=None) == ERR_ARG and snap(p=None) == ERR_ARG and snap(hh=None) == ERR_ARG
    assert snap(p=fs.SdfParams(2.0, 2.5)) == ERR_ARG and snap(f=fs.SdfFilter(5, 1, 0.0)) == ERR_ARG
    assert fs.lib.fluid_render_wait(h, None) == ERR_ARG
    assert fs.lib.fluid_render_wait(h, C.byref(img)) == ERR_STATE                   # a refused snapshot is not outstanding
    assert sim.render_stats() == {"pixels": 0, "hits": 0, "bytes_to_host": 0}

    p1 = fs.water_cube_drop(n, 4, seed=0)
    sim.upload_particles(p1)
    v1, _, bg = rs.level_set(p1, n, R, w, dx)
    r1 = rr.render(v1, bg, good, *rs.SHADE)
    sh = fs.Shade(f3(*rs.SHADE[0]), b3(*rs.SHADE[1]), 0)
    assert snap(sh=sh) == 0                                                         # q: everything
    sim.step()
    p2, _ = sim.download_particles()
    small = rs.pinhole(width=21, height=13, fov=30.0)                               # 3 W H = 819: the rgb part is padded to 832
    assert snap(c=fs.camera(*small), what=3, sh=sh, p=fs.SdfParams(2.0, 2.0)) == 0  # q + 1: another size, set and choice of parts
    assert sim.render_stats()["bytes_to_host"] == 16 + 832 + 4 * 273 == bytes_to_host(small, 3)
    for what in (1, 7):
        assert snap(what=what) == ERR_STATE                                         # a third is refused
        assert "two render snapshots" in fs.lib.fluid_last_error().decode()
    i1, i2 = fs.ImageC(), fs.ImageC()
    assert fs.lib.fluid_render_wait(h, C.byref(i1)) == 0
    assert sim.render_stats()["hits"] == i1.n_hit == r1["n_hit"]
    assert fs.lib.fluid_render_wait(h, C.byref(i2)) == 0
    assert fs.lib.fluid_render_wait(h, C.byref(i2)) == ERR_STATE
    view = lambda p, t, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=shape)   # noqa: E731
    # snapshot q's pointers are intact after snapshot q + 1 and both waits; the record's parts start at multiples of 16 / 4
    assert (i1.width, i1.height) == (48, 32) and i1.rgb % 16 == 0 and i1.depth == i1.rgb + 3 * 48 * 32 and i1.normals == i1.depth + 4 * 48 * 32
    assert np.array_equal(view(i1.rgb, C.c_uint8, (32, 48, 3)), r1["rgb"]) and np.array_equal(view(i1.depth, C.c_uint32, (32, 48)), rs.u32(r1["depth"]))
    assert np.array_equal(view(i1.normals, C.c_uint32, (32, 48, 3)), rs.u32(r1["normals"]))
    v2 = rs.level_set(p2, n, 2.0, 2.0, 1.0)[0]
    r2 = rr.render(v2, sdf_ref.constants(2.0, 2.0, 1.0)[3], small, *rs.SHADE)
    assert (i2.width, i2.height, i2.normals, i2.n_hit) == (21, 13, None, r2["n_hit"]) and i2.depth == i2.rgb + 832 and r2["n_hit"] > 20
    assert np.array_equal(view(i2.rgb, C.c_uint8, (13, 21, 3)), r2["rgb"]) and np.array_equal(view(i2.depth, C.c_uint32, (13, 21)), rs.u32(r2["depth"]))
    # the slots reused in both orders, two outstanding each time, sizes that grow and shrink
    va, _, bga = rs.level_set(p2, n, R, w, dx)
    cams = [good, small, rs.pinhole(width=7, height=5), good]
    refs = [rr.render(va, bga, c, *rs.SHADE) for c in cams]
    for a in range(len(cams) - 1):
        sim.render_snapshot(R, w, fs.camera(*cams[a]), shade=rs.SHADE, depth=True, normals=True)
        sim.render_snapshot(R, w, fs.camera(*cams[a + 1]), shade=rs.SHADE, depth=True, normals=True)
        rs.same(sim.render_wait(), refs[a], note=a)
        rs.same(sim.render_wait(), refs[a + 1], note=a)
    sim.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    h = sim._h
    cam = fs.camera(*rs.named_camera("cloud", n))
    for what in (1, 2, 4, 7):
        assert fs.lib.fluid_render_snapshot(h, C.byref(fs.SdfParams(1.5, 2.5)), None, C.byref(cam), None, what) == ERR_STATE
        msg = fs.lib.fluid_last_error().decode()
        assert "single-GPU" in msg and "fluid_sdf_grids_merge" in msg and "fluid_sdf_render" in msg
    assert fs.lib.fluid_render_wait(h, C.byref(fs.ImageC())) == ERR_STATE
    v = [C.c_int64() for _ in range(3)]
    assert fs.lib.fluid_render_stats(h, *[C.byref(x) for x in v]) == ERR_STATE
    sim.close()
    grp.close()


def test_density_surface_mesh_and_image_in_one_step(fs):
    """The four kinds have rings of their own: two of each can be outstanding at once, and each comes back as if taken alone."""
    n, (R, w, dx) = 32, SETS[0]
    cam = rs.pinhole(eye=(-30.0, 25.0, -40.0))
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, 4, seed=0))
    alone = []
    for k in range(2):
        sim.step()
        p, _ = sim.download_particles()
        val, act, bg = rs.level_set(p, n, R, w, dx)
        alone.append((rr.render(val, bg, cam, *rs.SHADE), sdf_ref.leaf_list(val, act, bg)))
        sim.output_snapshot()
        sim.sdf_snapshot(R, w)
        sim.mesh_snapshot(R, w, normals=True)
        sim.render_snapshot(R, w, fs.camera(*cam), shade=rs.SHADE, depth=True, normals=True)
    for k in range(2):
        assert sim.output_wait().n_leaves > 0
        g = sim.sdf_wait()
        assert np.array_equal(g.origin, alone[k][1][0]) and np.array_equal(rs.u32(g.values), rs.u32(alone[k][1][1]))
        v, q, parts = sim.mesh_wait_ex()
        assert len(q) > 100 and parts["normals"].shape == v.shape
        rs.same(sim.render_wait(), alone[k][0], note=k)
        assert alone[k][0]["n_hit"] > 100
    sim.close()


def test_snapshots_do_not_disturb_the_steps(fs):
    """A handle that renders after every step and one that never does end 3 steps with equal particles and stats."""
    n, (R, w, _) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=3)
    cam = fs.camera(*rs.pinhole(eye=(-30.0, 25.0, -40.0)))
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    for s in (a, b):
        s.upload_particles(pos)
    sa, sb = [], []
    for k in range(3):
        sa.append(a.step())
        sb.append(b.step())
        b.render_snapshot(R, w, cam, smooth=(1, 1, -0.25) if k == 1 else None, depth=k == 2)
        out = b.render_wait()
        assert out["n_hit"] > 100 and out["rgb"].shape == (32, 48, 3) and (out["depth"] is not None) == (k == 2)
    assert sa == sb
    (pa, va), (pb, vb) = a.download_particles(), b.download_particles()
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    a.close()
    b.close()


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


DRIVER_VARS = ("FLUID_OUT_MESH", "FLUID_OUT_MESH_VEL", "FLUID_OUT_SURFACE", "FLUID_OUT_DENSE", "FLUID_BLOCKS", "FLUID_BLOCKS_SURFACE", "FLUID_SOURCE_EVERY",
               "FLUID_RAW", "FLUID_OUT_SMOOTH", "FLUID_OUT_MESH_NORMALS", "FLUID_OUT_MESH_TRIS", "FLUID_BLOCKS_MESH", "FLUID_BLOCKS_MESH_VEL",
               "FLUID_BLOCKS_MESH_NORMALS", "FLUID_BLOCKS_MESH_TRIS", "FLUID_OUT_RENDER", "FLUID_OUT_RENDER_EYE", "FLUID_BLOCKS_RENDER",
               "FLUID_REBALANCE_EVERY", "FLUID_DIST_SOLVE", "FLUID_DEVICES")


def run_driver(d, **env):
    d.mkdir()
    e = {k: v for k, v in os.environ.items() if k not in DRIVER_VARS}
    e.update(FLUID_OUT=str(d / "simulation"), **{k: str(v) for k, v in env.items()})
    r = subprocess.run([os.path.join(ROOT, "fluid-simulation_amd", "fluid")], capture_output=True, text=True, env=e, cwd=d, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]


def files(d):
    return sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())


def test_driver_writes_frames(fs, tmp_path):
    """The `fluid` program with FLUID_OUT_RENDER (default size, a given eye, smoothed): frame<i>.png holds the pixels the handle gives
    for the same scene through fluid_camera_look_at; without the variables stdout and every file are what they were."""
    import leaf_ref
    n, ppc, steps, (R, w, dx), eye, filt = 24, 4, 2, SETS[0], (-25.0, 20.0, -28.0), (1, 1, -0.25)
    common = dict(FLUID_N=n, FLUID_PPC=ppc, FLUID_STEPS=steps)
    base = run_driver(tmp_path / "base", **common)
    more = run_driver(tmp_path / "more", FLUID_OUT_RENDER=f"{R},{w}", FLUID_OUT_RENDER_EYE=",".join(map(str, eye)),
                      FLUID_OUT_SMOOTH=",".join(map(str, filt)), **common)
    assert base == more
    frames = [f"simulation/frame{i}.png" for i in range(steps)]
    assert files(tmp_path / "more") == sorted(files(tmp_path / "base") + frames)
    for nm in files(tmp_path / "base"):
        assert leaf_ref.same_file(tmp_path / "base" / nm, tmp_path / "more" / nm), nm
    cam = fs.camera_look_at(n, eye)
    assert (cam.width, cam.height) == (640, 360)
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    for i in range(steps):
        sim.step()
        sim.render_snapshot(R, w, cam, smooth=filt)
        out = sim.render_wait()
        assert 0.02 < out["n_hit"] / (640 * 360) < 0.9
        assert np.array_equal(read_png(tmp_path / "more" / frames[i]), out["rgb"]), i
    sim.close()
    # refusals, before any handle is created
    exe = os.path.join(ROOT, "fluid-simulation_amd", "fluid")
    e = {k: v for k, v in os.environ.items() if k not in DRIVER_VARS}
    for bad in (dict(FLUID_OUT_RENDER="1.5"), dict(FLUID_OUT_RENDER="1.5,2.5,640"), dict(FLUID_OUT_RENDER="1.5,2.5,0x4"), dict(FLUID_OUT_RENDER="1.5,2.5x"),
                dict(FLUID_OUT_RENDER="1.5,2.5", FLUID_OUT_RENDER_EYE="1,2"), dict(FLUID_OUT_RENDER="1.5,2.5", FLUID_OUT_RENDER_EYE="0,9,0"),
                dict(FLUID_OUT_RENDER="1.5,2.5", FLUID_BLOCKS="2x1x1"), dict(FLUID_BLOCKS_RENDER="1.5,2.5"),
                dict(FLUID_BLOCKS="2x1x1", FLUID_BLOCKS_RENDER="1.5,2.5", FLUID_BLOCKS_MESH="2,2")):
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(e, FLUID_N="16", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "x"), **bad), cwd=tmp_path, timeout=60)
        assert r.returncode == 1 and "RENDER" in r.stderr and not (tmp_path / "x").exists(), bad


def test_block_driver_writes_frames(fs, tmp_path):
    """FLUID_BLOCKS=2x1x1 with FLUID_BLOCKS_RENDER (a given size, the default eye, smoothed): frame<i>.png is the reference's image of
    the particles the same block run has after each step; stdout and every other file are what they are without it."""
    import leaf_ref
    fd = fs.load_dist()
    n, ppc, steps, (R, w, dx), blocks, filt = 32, 2, 2, SETS[0], "2x1x1", (1, 2, -0.25)
    common = dict(FLUID_N=n, FLUID_PPC=ppc, FLUID_STEPS=steps, FLUID_BLOCKS=blocks)
    base = run_driver(tmp_path / "base", **common)
    more = run_driver(tmp_path / "more", FLUID_BLOCKS_RENDER=f"{R},{w},48x32", FLUID_OUT_SMOOTH=",".join(map(str, filt)), **common)
    assert base == more
    frames = [f"simulation/frame{i}.png" for i in range(steps)]
    assert files(tmp_path / "more") == sorted(files(tmp_path / "base") + frames)
    for nm in files(tmp_path / "base"):
        assert leaf_ref.same_file(tmp_path / "base" / nm, tmp_path / "more" / nm), nm
    # the same run here: the program's cut planes, ids and upload
    dims = (2, 1, 1)
    pos = fs.water_cube_drop(n, ppc, seed=0)
    grp = fd.LocalGroup(2)
    sims = [None] * 2

    def run(r):
        sims[r] = sim = fd.DistFluidSim(n, dims, fd.partition_blocks(n, pos, dims), grp.comms[r])
        sim.upload_global(pos)
        out = []
        for _ in range(steps):
            sim.step()
            out.append(sim.download_local())
        return out

    try:
        res = grp.run(run)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    c = fs.camera_look_at(n, (-0.9 * n, 0.5 * n, -1.2 * n), width=48, height=32)
    cam = rr.camera(list(c.eye), list(c.dir00), list(c.du), list(c.dv), c.width, c.height, c.t_near, c.step, c.n_steps)
    for i in range(steps):
        p = np.concatenate([r[i][0] for r in res])
        val, act, bg = rs.level_set(p, n, R, w, dx, filt)
        ref = rr.render(val, bg, cam)
        assert 0.02 < ref["n_hit"] / (48 * 32) < 0.9
        assert np.array_equal(read_png(tmp_path / "more" / frames[i]), ref["rgb"]), i
