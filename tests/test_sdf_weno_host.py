"""CPU (-m "not gpu"): the host half of the HJWENO5 renormalisation — fluid_sdf_filter_tracked, fluid_sdf_filter_grown and
fluid_sdf_flow with scheme FLUID_SDF_TRACK_HJWENO5 on tests/sdf_ref.py leaf lists against tests/sdf_weno_ref.py (origins, masks,
values as bit patterns, kept; ids and velocity bits where attributes travel), the sphere's offset drift through the C interface,
the refusals, FIRST_BIAS unchanged beside it, the driver's FLUID_OUT_TRACK_SCHEME, and the file under ASan + UBSan as a stand-alone
program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_flow_ref
import sdf_grow_ref
import sdf_ref
import sdf_track_ref
import sdf_weno_ref as W
from sdf_testlib import grid_of, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid-simulation_amd", "csrc")
ERR_ARG = 1
SCENES = ["one", "corner", "lo", "hi", "cloud"]
HJ = W.HJWENO5


def same_list(out, val, act, bg):
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    return out.n_leaves == len(org) and np.array_equal(out.origin, org) and np.array_equal(out.active, a) and np.array_equal(u32(out.values), u32(v))


@pytest.mark.parametrize("R,w,dx", mesh_ref.SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", SCENES)
def test_tracked_filter_is_the_reference(fs, name, n, R, w, dx):
    g = grid_of(fs, name, n, R, w, dx)
    assert g.n_leaves > 0
    for case in W.CASES:
        Wd, K, units, N, tr = case
        vt, at, bg, _ = W.scene(name, n, R, w, dx, case)
        filt = (Wd, K, units * dx)
        first = fs.sdf_filter_tracked(g, filt, (N, bool(tr)))
        out, kept = fs.sdf_filter_tracked(g, filt, (N, bool(tr), "hjweno5"))
        assert same_list(out, vt, at, bg), case
        assert np.array_equal(g.origin[kept], out.origin) and (np.diff(kept) > 0).all(), case
        dv, da = fs.sdf_to_dense(out)
        assert np.array_equal(u32(dv), u32(vt)) and np.array_equal(da, at), case
        # scheme 0 after scheme 4 on the same inputs: the bytes it gave before
        again = fs.sdf_filter_tracked(g, filt, (N, bool(tr), 0))
        assert np.array_equal(again[0].origin, first[0].origin) and np.array_equal(u32(again[0].values), u32(first[0].values))
        assert np.array_equal(again[0].active, first[0].active) and np.array_equal(again[1], first[1])


@pytest.mark.parametrize("R,w,dx", mesh_ref.SETS)
@pytest.mark.parametrize("n", [16, 25])
@pytest.mark.parametrize("name", SCENES)
def test_grown_filter_and_flows_are_the_reference(fs, name, n, R, w, dx):
    _, _, val, act, ids, v32, bg = sdf_grow_ref.base(name, n, R, w, dx)
    fR, fw = sdf_ref.constants(R, w, dx)[:2]
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    g = fs.SdfGrid(n, org, v, a, bg, fR, fw)
    attr = fs.SdfAttr(*attr_ref.leaf_attr(ids, v32, org))
    for Wd, K, units, N, tr in W.CASES:
        if not tr:
            continue                                     # growing requires the trim
        vt, at, it, velt = W.grown(val, act, bg, dx, Wd, K, units * dx, N, ids, v32)
        out, oa = fs.sdf_filter_grown(g, (Wd, K, units * dx), (N, True, HJ), attr=attr)
        assert same_list(out, vt, at, bg), (Wd, K, units, N)
        li, lv = attr_ref.leaf_attr(it, velt, out.origin)
        assert np.array_equal(oa.id, li) and np.array_equal(u32(oa.velocity), u32(lv)), (Wd, K, units, N)
        plain = fs.sdf_filter_grown(g, (Wd, K, units * dx), (N, True, HJ))
        assert same_list(plain, vt, at, bg)
    # one median and one mean-curvature flow: tracked with an offset, and grown
    for kind, grow, units in ((sdf_flow_ref.MEDIAN, False, 0.6), (sdf_flow_ref.CURVATURE, True, -0.6)):
        vt, at, _, _ = W.flow(kind, val, act, bg, dx, 1, 2, units * dx, 3, True, grow)
        out = fs.sdf_flow(g, kind, (1, 2, units * dx), track=(3, True, "hjweno5"), grow=grow)
        assert same_list(out, vt, at, bg), (kind, grow)


def sphere_grid(fs, R):
    val, act, d = W.sphere(R)
    org, v, a = sdf_ref.leaf_list(val, act, W.SPHERE_BG)
    return fs.SdfGrid(W.SPHERE_N, org, v, a, W.SPHERE_BG, 1.0, W.SPHERE_BG), val, act, d


@pytest.mark.parametrize("off", [0.5, -0.5])
@pytest.mark.parametrize("R", W.SPHERE_RADII)
def test_offset_sphere_through_the_c_interface(fs, R, off):
    """An exact sphere, offset by half a voxel (one step) and tracked once: the error against d + off over |d + off| < 1.5 is at
    most a fifth of the first-order reference's, and the bytes are the reference's."""
    g, val, act, d = sphere_grid(fs, R)
    out, _ = fs.sdf_filter_tracked(g, (1, 0, off), (3, True, "hjweno5"))
    dv, da = fs.sdf_to_dense(out)
    vr, ar = W.tracked(val, act, W.SPHERE_BG, 1.0, 1, 0, off, 3, True)
    assert np.array_equal(u32(dv), u32(vr)) and np.array_equal(da, ar)
    v1, a1 = sdf_track_ref.tracked(val, act, W.SPHERE_BG, 1.0, 1, 0, off, 3, True)
    m, m1 = da & (np.abs(d + off) < 1.5), a1 & (np.abs(d + off) < 1.5)
    e = float(np.abs(dv.astype(np.float64)[m] - (d + off)[m]).max())
    e1 = float(np.abs(v1.astype(np.float64)[m1] - (d + off)[m1]).max())
    print(f"R={R} off={off}: first {e1:.5f} hjweno5 {e:.5f} ratio {e1 / e:.1f}")
    assert e <= e1 / 5


def raw_tracked(fs, g, filt, track, cap, org, val, act, kept):
    c, _keep = g._c()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    f, t = fs.SdfFilter(*filt), fs.SdfTrack(*track)
    return fs.lib.fluid_sdf_filter_tracked(C.byref(c), C.byref(f), C.byref(t), cap, p(org), p(val), p(act), p(kept))


def test_refusals(fs):
    R, w, dx = mesh_ref.SETS[0]
    g = grid_of(fs, "hi", 25, R, w, dx)
    k0 = g.n_leaves
    org, val, act, kept = np.full((k0, 3), 7, np.int32), np.full((k0, 512), 7, np.float32), np.full((k0, 8), 7, np.uint64), np.full(k0, 7, np.int32)
    filt = (1, 1, 0.0)
    assert raw_tracked(fs, g, filt, (3, 1, HJ), 0, None, None, None, None) >= 0
    for scheme in (-1, 1, 2, 3, 5):
        assert raw_tracked(fs, g, filt, (3, 1, scheme), k0, org, val, act, kept) == -ERR_ARG, scheme
        assert raw_tracked(fs, g, filt, (3, 1, scheme), 0, None, None, None, None) == -ERR_ARG, scheme
        with pytest.raises(fs.FluidError):
            fs.sdf_filter_grown(g, filt, (3, True, scheme))
        with pytest.raises(fs.FluidError):
            fs.sdf_flow(g, sdf_flow_ref.MEDIAN, filt, track=(3, True, scheme))
    # whatever the tracked functions already refuse, under the new scheme
    for bad in ((-1, 1, HJ), (9, 1, HJ), (3, 2, HJ), (3, -1, HJ)):
        assert raw_tracked(fs, g, filt, bad, k0, org, val, act, kept) == -ERR_ARG, bad
    for bad in ((0, 1, 0.0), (5, 1, 0.0), (1, 17, 0.0), (1, 1, float("nan"))):
        assert raw_tracked(fs, g, bad, (3, 1, HJ), k0, org, val, act, kept) == -ERR_ARG, bad
    bg = float(g.background)
    assert raw_tracked(fs, g, (1, 1, bg * 1.01), (3, 1, HJ), k0, org, val, act, kept) == -ERR_ARG          # |off| > bg, tracked
    assert raw_tracked(fs, g, filt, (3, 1, HJ), 3, org, val, act, kept) == -ERR_ARG                        # cap too small
    assert raw_tracked(fs, g, filt, (3, 1, HJ), k0, org, None, act, kept) == -ERR_ARG                      # some but not all outputs
    with pytest.raises(fs.FluidError):
        fs.sdf_filter_grown(g, filt, (3, False, HJ))                                                        # growing needs the trim
    with pytest.raises(fs.FluidError):
        fs.sdf_filter_grown(g, (1, 1, 4.5 * dx), (3, True, HJ))
    assert (org == 7).all() and (val == 7).all() and (act == 7).all() and (kept == 7).all()
    with pytest.raises(ValueError):
        fs.sdf_filter_tracked(g, filt, (3, True, "weno"))
    assert fs.SDF_TRACK_SCHEMES == {"first": 0, "hjweno5": 4}


@pytest.mark.parametrize("extra", [{"FLUID_OUT_TRACK_SCHEME": "weno"}, {"FLUID_OUT_TRACK_SCHEME": "4"}, {"FLUID_OUT_TRACK_SCHEME": "HJWENO5"},
                                   {"FLUID_OUT_TRACK_SCHEME": "hjweno5", "FLUID_OUT_TRACK": ""}])
def test_driver_refuses_a_scheme_it_would_not_run(fs, tmp_path, extra):
    """FLUID_OUT_TRACK_SCHEME with another word, or without FLUID_OUT_TRACK: refused before any handle is created — the message is
    the variable's own, not the missing device's."""
    env = dict(os.environ, FLUID_N="16", FLUID_PPC="1", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "simulation"), FLUID_OUT_MESH="1.5,2.5",
               FLUID_OUT_SMOOTH="1,1", FLUID_OUT_TRACK="3")
    for k in ("FLUID_OUT_DENSE", "FLUID_BLOCKS", "FLUID_SOURCE_EVERY", "FLUID_RAW", "FLUID_OUT_SURFACE", "FLUID_BLOCKS_SURFACE", "FLUID_BLOCKS_MESH",
              "FLUID_BLOCKS_MESH_VEL", "FLUID_OUT_SMOOTH_KIND"):
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run([os.path.join(ROOT, "fluid-simulation_amd", "fluid")], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and "FLUID_OUT_TRACK_SCHEME" in r.stderr and "fluid_create" not in r.stderr, (r.returncode, r.stderr[-500:])
    assert not list(tmp_path.rglob("*.ply")) and not list(tmp_path.rglob("*.vdb"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_weno_host_functions_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_san_weno"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "sdf_filter_host.cpp"),
           os.path.join(ROOT, "tests", "host_san_weno_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host sanitizer run (weno): ok" in r.stdout
