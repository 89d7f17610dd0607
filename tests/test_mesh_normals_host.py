"""CPU (-m "not gpu"): the host half of the mesh's normals and triangles — fluid_sdf_mesh_normals and fluid_mesh_triangles on
tests/sdf_ref.py leaf lists against tests/mesh_normals_ref.py (floats as bit patterns), filtered lists, a hand-made list with a NaN
and an all-equal cell, the empty list, refusals, counts-only calls and caps too small, fluid_write_ply_mesh_ex re-read with numpy,
the driver's refusals, and all three host functions under ASan + UBSan as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_normals_ref as mn
import mesh_ref
import sdf_ref
from sdf_testlib import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid-simulation_amd", "csrc")
ERR_ARG = 1
SETS = mesh_ref.SETS
N = 32
FILTERS = [None, (1, 1, 0.0), (1, 4, -0.5), (1, 0, -0.9)]
NRM = "property float nx\nproperty float ny\nproperty float nz\n"
VEL = "property float vx\nproperty float vy\nproperty float vz\n"
HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
          "{nrm}{vel}element face {nf}\nproperty list uchar uint vertex_indices\nend_header\n")


def grid_of(fs, val, act, n, R, w, dx):
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    return fs.SdfGrid(n, org, v, a, bg, fR, fw)


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner", "lo", "hi", "cloud"])
def test_host_functions_are_the_reference(fs, name, R, w, dx):
    _, _, act, _ = mesh_ref.scene(name, N, R, w, dx)
    for filt in FILTERS:
        val, (vert, quads, _), nr, _, tri = mn.scene(name, N, R, w, dx, filt)
        g = grid_of(fs, val, act, N, R, w, dx)
        got = fs.sdf_mesh_normals(g)
        assert got.shape == nr.shape and np.array_equal(u32(got), u32(nr)), (name, filt)
        m = fs.sdf_mesh(g)
        assert np.array_equal(u32(m.vertices), u32(vert)) and np.array_equal(m.quads, quads)
        assert np.array_equal(fs.mesh_triangles(m.vertices, m.quads), tri), (name, filt)
        assert filt is not None or len(vert) > 0


def hand_made(n=16):
    """A block of -bg in +bg with a few values on and beside its faces, one of them NaN, and far from it a cell whose corners are a
    checkerboard of -1 / +1: mixed, every edge counts with t = 0.5, and each of the three sums cancels exactly — the gradient is
    zero.  (A cell whose eight corners are all equal is not mixed and has no vertex; this is the cell whose DIFFERENCES are all
    equal in size.)"""
    lo = sdf_ref.geometry(n)[0]
    bg = np.float32(2.0)
    val = np.full((n, n, n), bg, np.float32)
    b = slice(-2 - lo, 2 - lo)
    val[b, b, b] = -bg
    for x, y, z, v in [(-2, -1, 0, -0.5), (-3, -1, 0, 0.7), (1, 1, 1, -1.25), (1, 1, 2, 0.4), (0, 2, 0, np.nan), (-1, -3, -1, 0.3), (-2, -2, -2, -0.125)]:
        val[x - lo, y - lo, z - lo] = v
    # a cell far from the block, min corner (4, 4, 4): a checkerboard of -1 / +1 — mixed, and every one of the three sums cancels
    for d in np.ndindex(2, 2, 2):
        val[4 + d[0] - lo, 4 + d[1] - lo, 4 + d[2] - lo] = -1.0 if sum(d) % 2 == 0 else 1.0
    return val, bg


def test_hand_made_list_with_a_nan_and_a_vanishing_gradient(fs):
    n = 16
    val, bg = hand_made(n)
    vert, quads, cells, _ = mesh_ref.mesh(val)
    nr, ln = mn.normals(val)
    k = int(np.flatnonzero((cells == 4).all(axis=1))[0])
    assert ln[k] == 0 and np.isnan(ln).sum() >= 4                                 # the checkerboard cell; the cells round the NaN
    zero = ~(ln > 0)
    assert (u32(nr[zero]) == 0).all() and zero.sum() >= 5                         # +0.0f, never -0.0f, never NaN
    assert np.isfinite(nr).all()
    org, lv, la = sdf_ref.leaf_list(val, val != bg, bg)
    g = fs.SdfGrid(n, org, lv, la, bg, 3.0, 1.0)
    got = fs.sdf_mesh_normals(g)
    assert got.shape == nr.shape and np.array_equal(u32(got), u32(nr))
    tri, _ = mn.triangles(vert, quads)                                            # (the NaN voxel makes NaN vertices: ties' branch)
    assert np.isnan(vert).any()
    assert np.array_equal(fs.mesh_triangles(vert, quads), tri)


def test_empty_list_and_empty_mesh(fs):
    g = fs.SdfGrid(16, np.empty((0, 3)), np.empty((0, 512)), np.empty((0, 512)), 2.5, 1.5, 2.5)
    assert fs.sdf_mesh_normals(g).shape == (0, 3)
    assert fs.mesh_triangles(np.empty((0, 3)), np.empty((0, 4))).shape == (0, 3)
    m = fs.Mesh(16, np.empty((0, 3)), np.empty((0, 4)))._c()
    assert fs.lib.fluid_mesh_triangles(C.byref(m), 0, None) == 0


def test_refusals_counts_only_and_caps(fs):
    n, (R, w, dx) = N, SETS[1]
    val, (vert, quads, _), nr, _, tri = mn.scene("corner", n, R, w, dx)
    _, _, act, _ = mesh_ref.scene("corner", n, R, w, dx)
    g = grid_of(fs, val, act, n, R, w, dx)
    nv, nq = len(vert), len(quads)
    c, _keep = g._c()
    f = fs.lib.fluid_sdf_mesh_normals
    assert f(C.byref(c), 0, None) == nv                                            # the count only: the cap is ignored
    out = np.full((nv + 2, 3), 7, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    assert f(C.byref(c), nv - 1, p) == -ERR_ARG                                    # a cap too small
    assert f(None, nv, p) == -ERR_ARG
    for o in (g.origin[[0, 2, 1] + list(range(3, g.n_leaves))], g.origin + np.int32([0, 4, 0])):   # unsorted; off the 8-grid
        bad, _k2 = fs.SdfGrid(n, o, g.values, g.active, g.background, g.radius, g.half_width)._c()
        assert f(C.byref(bad), nv, p) == -ERR_ARG
    assert (out == 7).all()                                                        # nothing written
    assert f(C.byref(c), nv + 2, p) == nv
    assert np.array_equal(u32(out[:nv]), u32(nr)) and (out[nv:] == 7).all()

    t = fs.lib.fluid_mesh_triangles
    m = fs.Mesh(n, vert, quads)
    assert t(C.byref(m._c()), 0, None) == 2 * nq
    tout = np.full((2 * nq + 2, 3), 9, np.uint32)
    tp = tout.ctypes.data_as(C.c_void_p)
    assert t(C.byref(m._c()), 2 * nq - 1, tp) == -ERR_ARG                          # a cap too small
    assert t(None, 2 * nq, tp) == -ERR_ARG
    q = quads.copy()
    q[3, 2] = nv
    assert t(C.byref(fs.Mesh(n, vert, q)._c()), 2 * nq, tp) == -ERR_ARG            # an entry >= n_vertices
    assert t(C.byref(fs.Mesh(n, vert, q)._c()), 0, None) == -ERR_ARG               # ... also when only the count is asked for
    mc = m._c()
    assert t(C.byref(fs.MeshC(n, nv, nq, 0, 0, 0, None, mc.quads)), 2 * nq, tp) == -ERR_ARG      # counts without their arrays
    assert t(C.byref(fs.MeshC(n, nv, nq, 0, 0, 0, mc.vertices, None)), 2 * nq, tp) == -ERR_ARG
    assert t(C.byref(fs.MeshC(n, -1, nq, 0, 0, 0, mc.vertices, mc.quads)), 2 * nq, tp) == -ERR_ARG
    assert (tout == 9).all()                                                       # nothing written
    assert t(C.byref(m._c()), 2 * nq + 2, tp) == 2 * nq
    assert np.array_equal(tout[:2 * nq], tri) and (tout[2 * nq:] == 9).all()
    with pytest.raises(fs.FluidError):
        fs.mesh_triangles(vert, q)


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii")
    nv = int(head.split("element vertex ")[1].split("\n")[0])
    nf = int(head.split("element face ")[1].split("\n")[0])
    k = 3 + 3 * ("property float nx\n" in head) + 3 * ("property float vx\n" in head)
    v = np.frombuffer(raw, "<f4", k * nv, end).reshape(nv, k)
    rest = len(raw) - end - 4 * k * nv
    per = 3 if nf and rest == 13 * nf else 4
    f = np.frombuffer(raw, np.dtype([("k", "u1"), ("i", "<u4", per)]), nf, end + 4 * k * nv)
    assert end + 4 * k * nv + (1 + 4 * per) * nf == len(raw)
    return head, v, f


@pytest.mark.parametrize("what", range(8))
def test_ply_rereads(fs, tmp_path, what):
    """Records of 12, 24 and 36 bytes, quads or triangle faces, the header line by line."""
    n, prm, voxel, scale = N, (3.0, 1.0, 1.0), 0.3, -24.0
    _, (vert, quads, _), nr, _, tri = mn.scene("cloud", n, *prm)
    vv = np.random.default_rng(2).uniform(-3, 3, vert.shape).astype(np.float32)
    kw = {}
    if what & 1:
        kw.update(velocity=vv, velocity_scale=scale)
    if what & 2:
        kw.update(normals=nr)
    if what & 4:
        kw.update(triangles=tri)
    path = tmp_path / "m.ply"
    fs.write_ply_mesh(path, (vert, quads), voxel, **kw)
    head, v, f = read_ply(path)
    assert head == HEADER.format(nv=len(vert), nf=2 * len(quads) if what & 4 else len(quads), nrm=NRM if what & 2 else "", vel=VEL if what & 1 else "")
    assert v.shape[1] == 3 * (1 + (what & 1) + ((what >> 1) & 1))                  # 12, 24 or 36 bytes
    assert np.array_equal(u32(v[:, :3]), u32(vert * np.float32(voxel)))
    col = 3
    if what & 2:
        assert np.array_equal(u32(v[:, 3:6]), u32(nr))                             # unscaled
        col = 6
    if what & 1:
        assert np.array_equal(u32(v[:, col:col + 3]), u32(vv * np.float32(scale)))
    if what & 4:
        assert (f["k"] == 3).all() and np.array_equal(f["i"], tri)
    else:
        assert (f["k"] == 4).all() and np.array_equal(f["i"], quads)
    if what == 0:                                                                  # (no part: the plain writer's route and bytes)
        fs.write_ply_mesh(tmp_path / "p.ply", (vert, quads), voxel)
        ex = fs.MeshExC(None, None, None, 0)
        assert fs.lib.fluid_write_ply_mesh_ex(str(tmp_path / "x.ply").encode(), C.byref(fs.Mesh(0, vert, quads)._c()), C.byref(ex), voxel, 1.0) == 0
        assert fs.lib.fluid_write_ply_mesh_ex(str(tmp_path / "y.ply").encode(), C.byref(fs.Mesh(0, vert, quads)._c()), None, voxel, 1.0) == 0
        plain = open(tmp_path / "p.ply", "rb").read()
        assert plain == open(path, "rb").read() == open(tmp_path / "x.ply", "rb").read() == open(tmp_path / "y.ply", "rb").read()
    if what == 7:                                                                  # an empty mesh keeps the header lines
        fs.write_ply_mesh(tmp_path / "e.ply", fs.Mesh(16, np.empty((0, 3)), np.empty((0, 4))), voxel, velocity=np.empty((0, 3)),
                          normals=np.empty((0, 3)), triangles=np.empty((0, 3)))
        assert open(tmp_path / "e.ply", "rb").read().decode() == HEADER.format(nv=0, nf=0, nrm=NRM, vel=VEL)


def test_ply_refusals(fs, tmp_path):
    n, prm = N, SETS[0]
    _, (vert, quads, _), nr, _, tri = mn.scene("one", n, *prm)
    nv, nq = len(vert), len(quads)
    m = fs.Mesh(n, vert, quads)._c()
    w = fs.lib.fluid_write_ply_mesh_ex
    nrm, t = np.ascontiguousarray(nr), np.ascontiguousarray(tri)
    p = str(tmp_path / "m.ply").encode()
    ex = fs.MeshExC(None, nrm.ctypes.data, t.ctypes.data, 2 * nq)
    assert w(str(tmp_path / "no_such_dir" / "m.ply").encode(), C.byref(m), C.byref(ex), 1.0, 1.0) == ERR_ARG
    for vs in (0.0, -1.0, float("nan")):
        assert w(p, C.byref(m), C.byref(ex), vs, 1.0) == ERR_ARG, vs
    assert w(p, None, C.byref(ex), 1.0, 1.0) == ERR_ARG and w(None, C.byref(m), C.byref(ex), 1.0, 1.0) == ERR_ARG
    for k in (2 * nq - 1, 2 * nq + 1, nq, 0):
        assert w(p, C.byref(m), C.byref(fs.MeshExC(None, None, t.ctypes.data, k)), 1.0, 1.0) == ERR_ARG, k    # not twice the quads
    t2 = t.copy()
    t2[5, 1] = nv
    assert w(p, C.byref(m), C.byref(fs.MeshExC(None, None, t2.ctypes.data, 2 * nq)), 1.0, 1.0) == ERR_ARG     # an entry >= n_vertices
    q = quads.copy()
    q[3, 2] = nv
    assert w(p, C.byref(fs.Mesh(n, vert, q)._c()), C.byref(ex), 1.0, 1.0) == ERR_ARG
    vel = np.zeros((nv, 3), np.float32)
    for sc in (float("nan"), float("inf")):
        assert w(p, C.byref(m), C.byref(fs.MeshExC(vel.ctypes.data, nrm.ctypes.data, None, 0)), 1.0, sc) == ERR_ARG
    assert not (tmp_path / "m.ply").exists()
    assert w(p, C.byref(m), C.byref(ex), 1.0, float("nan")) == 0                   # no velocities: the scale is not looked at
    with pytest.raises(fs.FluidError):
        fs.write_ply_mesh(tmp_path / "n.ply", (vert, quads), 1.0, normals=nr[:-1])
    with pytest.raises(fs.FluidError):
        fs.write_ply_mesh(tmp_path / "n.ply", (vert, quads), 1.0, triangles=tri[:-1])
    assert not (tmp_path / "n.ply").exists()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_normals_host_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "normals_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "mesh_host.cpp"),
           os.path.join(ROOT, "tests", "host_san_normals_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host sanitizer run (normals): ok" in r.stdout
    nv, nq = (int(x) for x in r.stdout.split("ok")[1].split())
    head, v, f = read_ply(tmp_path / "san_normals7.ply")                         # what the sanitized build wrote re-reads too
    assert head == HEADER.format(nv=nv, nf=2 * nq, nrm=NRM, vel=VEL) and (f["k"] == 3).all() and f["i"].max() < nv and v.shape == (nv, 9)
    head, v, f = read_ply(tmp_path / "san_normals2.ply")
    assert head == HEADER.format(nv=nv, nf=nq, nrm=NRM, vel="") and (f["k"] == 4).all() and v.shape == (nv, 6)


BASE = {"FLUID_OUT_MESH_NORMALS": "FLUID_OUT_MESH", "FLUID_OUT_MESH_TRIS": "FLUID_OUT_MESH", "FLUID_BLOCKS_MESH_NORMALS": "FLUID_BLOCKS_MESH",
        "FLUID_BLOCKS_MESH_TRIS": "FLUID_BLOCKS_MESH"}


@pytest.mark.parametrize("value", ["1", "yes"])
@pytest.mark.parametrize("switch", sorted(BASE))
def test_driver_refuses_a_switch_without_its_base_or_malformed(fs, tmp_path, switch, value):
    """"1" without the base switch; a malformed value with it.  Refused before any handle is created (no GPU is touched)."""
    assert fs.lib.fluid_mesh_snapshot_ex
    env = dict(os.environ, FLUID_N="16", FLUID_PPC="1", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "simulation"))
    for k in ("FLUID_OUT_DENSE", "FLUID_BLOCKS", "FLUID_SOURCE_EVERY", "FLUID_RAW", "FLUID_OUT_SURFACE", "FLUID_BLOCKS_SURFACE", "FLUID_OUT_SMOOTH",
              "FLUID_OUT_MESH", "FLUID_OUT_MESH_VEL", "FLUID_BLOCKS_MESH", "FLUID_BLOCKS_MESH_VEL") + tuple(BASE):
        env.pop(k, None)
    env[switch] = value
    if value != "1":
        env[BASE[switch]] = "1.5,2.5"
        if "BLOCKS" in switch:
            env["FLUID_BLOCKS"] = "2x1x1"
    r = subprocess.run([os.path.join(ROOT, "fluid-simulation_amd", "fluid")], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and switch in r.stderr and BASE[switch] in r.stderr, (r.returncode, r.stderr[-500:])
    assert not list(tmp_path.rglob("*.ply")) and not list(tmp_path.rglob("*.vdb"))
