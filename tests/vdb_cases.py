"""What tests/test_vdb_ref.py, tests/test_gpu_vdb_ref.py and tests/golden/make_vdb_golden.py share — test infrastructure.

The fields the numpy references, the host library and the kernels are held to OpenVDB's own operators on (oracle/vdb_ref.py), and
the filter composed from those operators alone: no pass, constant or schedule of sdf_filter_ref, sdf_track_ref, sdf_weno_ref or
sdf_flow_ref is used here, so that a mistake in one of them cannot be on both sides of a comparison (scene_field() takes a scene's
particle positions from sdf_flow_ref.positions(), an input only).
  adversarial()   six fields no particle set gives: rough, tiny, flat, integer, huge, linear
  scene_field()   the unfiltered level set of a scene of tests/mesh_ref.py / sdf_flow_ref.py
  as_list_field() a field made fit for a leaf list: active values inside the band, inactive ones at +-bg
  iteration()     one filter iteration of a kind from OpenVDB's passes;  trim();  flow(): K iterations, each tracked
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from oracle.vdb_ref import FIRST, HJWENO5  # noqa: E402  (BiasedGradientScheme's numbers: one statement of them)

F = np.float32
BOX, MEDIAN, LAPLACIAN, CURVATURE = 0, 1, 2, 3
ADVERSARIAL = ("rough", "tiny", "flat", "integer", "huge", "linear")
DXS = (1.0, 0.5, 0.8)


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def clean(val):
    """No NaN, no inf, no -0.0: std::nth_element does not order signed zeros, and the key order that does is this project's own."""
    v = np.asarray(val)
    return bool(np.isfinite(v).all() and not (np.signbit(v) & (v == 0)).any())


def adversarial(n, dx, seed=7):
    """{name: (val, act, bg)}: about 85 % of the voxels active at random, bg = 3 dx."""
    rng = np.random.default_rng(seed)
    bg = F(F(dx) * F(3))
    act = rng.uniform(0, 1, (n, n, n)) < 0.85
    u = lambda: rng.uniform(-3, 3, (n, n, n))   # noqa: E731
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    fields = {
        "rough": u(),
        "tiny": u() * 1e-20,                                               # the WENO eps and Tolerance dominate
        "flat": np.where(rng.uniform(0, 1, (n, n, n)) < 0.7, 0.75, u()),   # the curvature's normGrad <= Tolerance branch
        "integer": np.round(u()) + 0.0,                                    # ties and zeros (+ 0.0: no -0.0)
        "huge": u() * 1e18,
        "linear": 0.25 * i - 0.5 * j + 0.125 * k - 1.0,                    # exactly linear in float32
    }
    out = {}
    for name in ADVERSARIAL:
        v = fields[name].astype(F)
        assert clean(v), name
        v.setflags(write=False)
        out[name] = (v, act, bg)
    act.setflags(write=False)
    return out


_scenes = {}


def scene_field(name, n, R, w, dx):
    """(val, act, bg) of an unfiltered scene; cached, read-only."""
    import sdf_flow_ref
    import sdf_ref
    key = (name, n, R, w, dx)
    if key not in _scenes:
        val, act = sdf_ref.closed(sdf_flow_ref.positions(name, n), n, R, w, dx)
        assert clean(val)
        val.setflags(write=False)
        act.setflags(write=False)
        _scenes[key] = (val, act, sdf_ref.constants(R, w, dx)[3])
    return _scenes[key]


SCENES = [("one", 16), ("corner", 16), ("cloud", 16), ("leafcorner", 32)]


def as_list_field(val, act, bg):
    """A field a leaf list can carry: active values clipped to +-0.99 bg, inactive voxels at +-bg by their sign."""
    bg = F(bg)
    lim = F(F(0.99) * bg)
    v = np.where(act, np.clip(val, -lim, lim), np.where(val < 0, -bg, bg)).astype(F)
    assert clean(v)
    return v


# ---- the filter from OpenVDB's passes alone ---------------------------------------------------------------------------------------
def iteration(ref, kind, val, act, bg, dx, W):
    if kind == BOX:
        for axis in ref.box_order()[0]:                    # tools/LevelSetFilter.h:303-310 through 231-233, as compiled
            val = ref.box_pass(val, act, bg, W, axis)
        return val
    if kind == MEDIAN:
        return ref.median_pass(val, act, bg, W)
    return ref.laplacian_pass(val, act, bg, dx) if kind == LAPLACIAN else ref.curvature_pass(val, act, bg, dx)


def trim(val, act, bg):
    """tools/LevelSetTracker.h:469-472: an active voxel at or beyond the background is set to it, by sign, and turned off."""
    neg, pos = act & (val <= -F(bg)), act & (val >= F(bg))
    val = np.where(neg, -F(bg), np.where(pos, F(bg), val)).astype(F)
    return val, act & ~neg & ~pos


def flow(ref, kind, val, act, bg, dx, W, K, N=0, do_trim=False, scheme=FIRST):
    """(val, act) after K iterations of `kind`, each followed (N > 0 or do_trim) by N normalise passes of `scheme` and the trim."""
    val, act = np.array(val, dtype=F), np.array(act, dtype=bool)
    for _ in range(K):
        val = iteration(ref, kind, val, act, bg, dx, W)
        for _ in range(N):
            val = ref.norm_pass(val, act, bg, dx, scheme)
        if do_trim:
            val, act = trim(val, act, bg)
    return val, act


# ---- the forms the GPU tests and the fixture share: (kind, W, N, trim, scheme) with K = 1 ---------------------------------------------
GPU_SET = (2.0, 2.0, 1.0)                                  # R, w, dx of the cloud, the leaf corner and the falling cube
GPU_FORMS = [(BOX, 1, 0, False, FIRST), (MEDIAN, 1, 0, False, FIRST), (MEDIAN, 2, 0, False, FIRST), (LAPLACIAN, 1, 0, False, FIRST),
             (CURVATURE, 1, 0, False, FIRST), (BOX, 1, 2, True, FIRST), (BOX, 1, 2, True, HJWENO5), (CURVATURE, 1, 2, True, FIRST),
             (CURVATURE, 1, 2, True, HJWENO5)]
FIXTURE_FORMS = [GPU_FORMS[0], GPU_FORMS[2], GPU_FORMS[5], GPU_FORMS[8]]   # those the fixture stores for the cloud
KIND_NAMES = {BOX: "box", MEDIAN: "median", LAPLACIAN: "laplacian", CURVATURE: "curvature"}
SCHEME_NAMES = {FIRST: "first", HJWENO5: "hjweno5"}


def form_name(form):
    kind, W, N, tr, scheme = form
    return f"{KIND_NAMES[kind]}{W}" + (f"_track{N}{int(tr)}_{SCHEME_NAMES[scheme]}" if N or tr else "")
