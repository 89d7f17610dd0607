"""CPU (-m "not gpu"): the host half of the liquid surface's attributes — fluid_sdf_mesh_attr and fluid_sdf_attr_to_dense on
tests/sdf_ref.py leaf lists with tests/attr_ref.py attributes against the reference (floats as bit patterns, ids exactly), a
hand-made list that reaches the rule for an edge with no active end, the refusals, the PLY writer re-read with numpy, the driver's
refusals, and all three host functions under ASan + UBSan as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_filter_ref
import sdf_ref
from sdf_testlib import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid-simulation_amd", "csrc")
ERR_ARG = 1
SETS = mesh_ref.SETS
FILTERS = [None] + sdf_filter_ref.FILTERS + [(1, 0, -0.9)]
HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
          "{vel}element face {nq}\nproperty list uchar uint vertex_indices\nend_header\n")
VEL = "property float vx\nproperty float vy\nproperty float vz\n"


def lists_of(fs, val, act, ids, v32, n, R, w, dx):
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    li, lv = attr_ref.leaf_attr(ids, v32, org)
    return fs.SdfGrid(n, org, v, a, bg, fR, fw), fs.SdfAttr(li, lv)


CASES = ([("one", n, s) for n in (16, 25) for s in SETS] +
         [("corner", 16, SETS[0]), ("corner", 16, SETS[1]), ("lo", 16, SETS[1]), ("lo", 25, SETS[0]), ("hi", 25, SETS[3]), ("hi", 16, SETS[1]),
          ("tie", 16, SETS[0]), ("cloud", 25, (3.0, 1.0, 1.0)), ("cloud", 25, (1.0, 1.0, 1.0))])


@pytest.mark.parametrize("name,n,prm", CASES)
def test_host_functions_are_the_reference(fs, name, n, prm):
    for filt in FILTERS:
        _, _, val, act, ids, v32, (vv, classes), mref = attr_ref.scene(name, n, *prm, filt)
        g, at = lists_of(fs, val, act, ids, v32, n, *prm)
        assert g.n_leaves > 0 and classes["vertices"] == len(mref[0]) and classes["none"] == 0
        assert filt is not None or len(mref[0]) > 0                              # (a filter may take a small ball's surface away)
        got = fs.sdf_mesh_attr(g, at)
        assert got.shape == vv.shape and np.array_equal(u32(got), u32(vv)), (name, filt)
        assert len(fs.sdf_mesh(g).vertices) == len(got)
        if filt is None:
            di, dv = fs.sdf_attr_to_dense(g, at)
            assert np.array_equal(di, ids) and np.array_equal(u32(dv), u32(v32))


def hand_made(n=16):
    """A block of inactive -bg in inactive +bg with a few active voxels on and beside its faces: most counting edges have no
    active end, some have one, a few have two."""
    lo = sdf_ref.geometry(n)[0]
    bg = np.float32(2.0)
    val = np.full((n, n, n), bg, np.float32)
    act = np.zeros((n, n, n), bool)
    vel = np.zeros((3, n, n, n), np.float32)
    ids = np.full((n, n, n), attr_ref.NO_ID, np.uint32)
    b = slice(-2 - lo, 2 - lo)
    val[b, b, b] = -bg
    rng = np.random.default_rng(11)
    for k, (x, y, z, v) in enumerate([(-2, -1, 0, -0.5), (-3, -1, 0, 0.7), (1, 1, 1, -1.25), (1, 1, 2, 0.4), (0, 2, 0, 1.5), (-1, -3, -1, 0.3),
                                      (-2, -2, -2, -0.125), (7, 7, 7, -0.5), (-8, -8, -8, -1.0), (-8, -8, -7, 0.25)]):
        i = (x - lo, y - lo, z - lo)
        val[i], act[i], ids[i] = v, True, 40 - k
        vel[(slice(None),) + i] = rng.uniform(-2, 2, 3).astype(np.float32)
    return val, act, ids, vel, bg


def test_hand_made_list_reaches_the_no_active_end_rule(fs):
    n = 16
    val, act, ids, vel, bg = hand_made(n)
    vv, classes = attr_ref.vertex_velocity(val, act, vel)
    assert classes["none"] > 50 and classes["one"] > 10 and classes["two"] >= 2
    assert classes["empty"] > 10 and classes["partial"] > 5                      # kv == 0 -> +0; only some edges contribute
    assert (u32(vv)[(vv == 0).all(axis=1)] == 0).all()                           # +0.0f, never -0.0f
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    li, lv = attr_ref.leaf_attr(ids, vel, org)
    g, at = fs.SdfGrid(n, org, v, a, bg, 3.0, 1.0), fs.SdfAttr(li, lv)
    got = fs.sdf_mesh_attr(g, at)
    assert got.shape == vv.shape == (classes["vertices"], 3) and np.array_equal(u32(got), u32(vv))
    assert int((got == 0).all(axis=1).sum()) >= classes["empty"]
    di, dv = fs.sdf_attr_to_dense(g, at)
    assert np.array_equal(di, ids) and np.array_equal(u32(dv), u32(vel))
    assert len(mesh_ref.mesh(val)[0]) == len(got)


def test_empty_list(fs):
    g = fs.SdfGrid(16, np.empty((0, 3)), np.empty((0, 512)), np.empty((0, 512)), 2.5, 1.5, 2.5)
    at = fs.SdfAttr(np.empty((0, 512)), np.empty((0, 3, 512)))
    assert fs.sdf_mesh_attr(g, at).shape == (0, 3)
    di, dv = fs.sdf_attr_to_dense(g, at)
    assert (di == attr_ref.NO_ID).all() and (u32(dv) == 0).all()


def test_refusals_and_count_only(fs):
    n, prm = 16, SETS[1]
    _, _, val, act, ids, v32, (vv, _), _ = attr_ref.scene("corner", n, *prm)
    g, at = lists_of(fs, val, act, ids, v32, n, *prm)
    nv = len(vv)
    c, _keep = g._c()
    a = at._c()
    f = fs.lib.fluid_sdf_mesh_attr
    assert f(C.byref(c), C.byref(a), 0, None) == nv                                # the count only: the cap is ignored
    out = np.full((nv + 2, 3), 7, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    assert f(C.byref(c), C.byref(a), nv - 1, p) == -ERR_ARG                        # a cap too small
    short = fs.SdfAttrC(g.n_leaves - 1, a.id, a.velocity)
    assert f(C.byref(c), C.byref(short), nv, p) == -ERR_ARG                        # attributes of another list
    assert f(C.byref(c), C.byref(fs.SdfAttrC(g.n_leaves, None, a.velocity)), nv, p) == -ERR_ARG
    assert f(C.byref(c), C.byref(fs.SdfAttrC(g.n_leaves, a.id, None)), nv, p) == -ERR_ARG
    assert f(C.byref(c), None, nv, p) == -ERR_ARG and f(None, C.byref(a), nv, p) == -ERR_ARG
    d = fs.lib.fluid_sdf_attr_to_dense
    di = np.full((n, n, n), 7, np.uint32)
    assert d(C.byref(c), C.byref(short), di.ctypes.data_as(C.c_void_p), None) == ERR_ARG
    for o in (g.origin[[0, 2, 1] + list(range(3, g.n_leaves))], g.origin + np.int32([0, 4, 0])):   # unsorted; off the 8-grid
        bad, _k2 = fs.SdfGrid(n, o, g.values, g.active, g.background, g.radius, g.half_width)._c()
        assert f(C.byref(bad), C.byref(a), nv, p) == -ERR_ARG
        assert d(C.byref(bad), C.byref(a), di.ctypes.data_as(C.c_void_p), None) == ERR_ARG
    assert (out == 7).all() and (di == 7).all()                                    # nothing written
    assert f(C.byref(c), C.byref(a), nv + 2, p) == nv
    assert np.array_equal(u32(out[:nv]), u32(vv)) and (out[nv:] == 7).all()
    assert d(C.byref(c), C.byref(a), None, None) == 0                              # either array may be NULL


def read_ply_vel(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii")
    nv = int(head.split("element vertex ")[1].split("\n")[0])
    nq = int(head.split("element face ")[1].split("\n")[0])
    v = np.frombuffer(raw, "<f4", 6 * nv, end).reshape(nv, 6)
    f = np.frombuffer(raw, np.dtype([("k", "u1"), ("i", "<u4", 4)]), nq, end + 24 * nv)
    assert end + 24 * nv + 17 * nq == len(raw)
    return head, v, f


@pytest.mark.parametrize("voxel_size,scale", [(1.0, 1.0), (0.3, 0.1), (0.5, -24.0)])
def test_ply_with_velocities_rereads(fs, tmp_path, voxel_size, scale):
    n, prm = 25, (3.0, 1.0, 1.0)
    _, _, val, act, ids, v32, (vv, _), (vert, quads, _, _) = attr_ref.scene("cloud", n, *prm)
    path = tmp_path / "m.ply"
    fs.write_ply_mesh(path, (vert, quads), voxel_size, velocity=vv, velocity_scale=scale)
    head, v, f = read_ply_vel(path)
    assert head == HEADER.format(nv=len(vert), nq=len(quads), vel=VEL)
    assert np.array_equal(u32(v[:, :3]), u32(vert * np.float32(voxel_size)))
    assert np.array_equal(u32(v[:, 3:]), u32(vv * np.float32(scale)))              # the scale applied in float
    assert (f["k"] == 4).all() and np.array_equal(f["i"], quads)
    # the plain writer's bytes for the same mesh are what they were: the header without the three lines, three floats per vertex
    fs.write_ply_mesh(tmp_path / "p.ply", (vert, quads), voxel_size)
    plain = open(tmp_path / "p.ply", "rb").read()
    assert plain == (HEADER.format(nv=len(vert), nq=len(quads), vel="").encode() + (vert * np.float32(voxel_size)).astype("<f4").tobytes()
                     + f.tobytes())
    fs.write_ply_mesh(tmp_path / "e.ply", fs.Mesh(16, np.empty((0, 3)), np.empty((0, 4))), voxel_size, velocity=np.empty((0, 3)))
    assert open(tmp_path / "e.ply", "rb").read().decode() == HEADER.format(nv=0, nq=0, vel=VEL)


def test_ply_with_velocities_refusals(fs, tmp_path):
    n, prm = 16, SETS[0]
    _, _, _, _, _, _, (vv, _), (vert, quads, _, _) = attr_ref.scene("one", n, *prm)
    m = fs.Mesh(n, vert, quads)._c()
    w = fs.lib.fluid_write_ply_mesh_attr
    vel = np.ascontiguousarray(vv)
    at = fs.MeshAttrC(len(vel), vel.ctypes.data)
    p = str(tmp_path / "m.ply").encode()
    assert w(str(tmp_path / "no_such_dir" / "m.ply").encode(), C.byref(m), C.byref(at), 1.0, 1.0) == ERR_ARG
    for vs, sc in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (1.0, float("nan")), (1.0, float("inf"))):
        assert w(p, C.byref(m), C.byref(at), vs, sc) == ERR_ARG, (vs, sc)
    assert w(p, C.byref(m), C.byref(fs.MeshAttrC(len(vel) - 1, vel.ctypes.data)), 1.0, 1.0) == ERR_ARG      # a vertex-count mismatch
    assert w(p, C.byref(m), C.byref(fs.MeshAttrC(len(vel), None)), 1.0, 1.0) == ERR_ARG
    assert w(p, C.byref(m), None, 1.0, 1.0) == ERR_ARG and w(p, None, C.byref(at), 1.0, 1.0) == ERR_ARG
    q = quads.copy(); q[3, 2] = len(vert)
    assert w(p, C.byref(fs.Mesh(n, vert, q)._c()), C.byref(at), 1.0, 1.0) == ERR_ARG
    assert not (tmp_path / "m.ply").exists()
    with pytest.raises(fs.FluidError):
        fs.write_ply_mesh(tmp_path / "m.ply", (vert, quads), 1.0, velocity=vv[:-1])
    assert w(p, C.byref(m), C.byref(at), 1.0, 0.0) == 0                                                     # a zero scale is a scale


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_attribute_host_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "attr_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "mesh_host.cpp"),
           os.path.join(ROOT, "tests", "attr_san_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host sanitizer run (attr): ok" in r.stdout
    nv, nq = (int(x) for x in r.stdout.split("ok")[1].split())
    head, v, f = read_ply_vel(tmp_path / "san_attr.ply")                         # what the sanitized build wrote re-reads too
    assert head == HEADER.format(nv=nv, nq=nq, vel=VEL) and (f["k"] == 4).all() and f["i"].max() < nv and np.isfinite(v).all()


@pytest.mark.parametrize("extra", [{"FLUID_OUT_MESH": ""}, {"FLUID_OUT_MESH_VEL": "fast"}, {"FLUID_OUT_MESH_VEL": "1,2"}, {"FLUID_OUT_MESH_VEL": "inf"},
                                   {"FLUID_BLOCKS": "2x1x1"}])
def test_driver_refuses_velocities_it_would_not_write(fs, tmp_path, extra):
    env = dict(os.environ, FLUID_N="16", FLUID_PPC="1", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "simulation"), FLUID_OUT_MESH="1.5,2.5",
               FLUID_OUT_MESH_VEL="1")
    for k in ("FLUID_OUT_DENSE", "FLUID_BLOCKS", "FLUID_SOURCE_EVERY", "FLUID_RAW", "FLUID_OUT_SURFACE", "FLUID_BLOCKS_SURFACE", "FLUID_OUT_SMOOTH"):
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run([os.path.join(ROOT, "fluid-simulation_amd", "fluid")], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and "FLUID_OUT_MESH" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not list(tmp_path.rglob("*.ply")) and not list(tmp_path.rglob("*.vdb"))
