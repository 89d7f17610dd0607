"""Reference for the HJWENO5 renormalisation of the liquid surface (include/fluid_hip.h, "liquid surface, renormalised: HJWENO5") —
test infrastructure, numpy only.

OpenVDB's LevelSetTracker::normalize() with HJWENO5_BIAS / TVD_RK1 (tools/LevelSetTracker.h:596-609; math/Operators.h:252-284;
math/FiniteDifference.h:331-349, 352-374, 1224-1233, 1428-1435) on a dense (val, act) (n, n, n) of tests/sdf_ref.py closed(): the grid
is padded by three voxels of +bg, a pass is Jacobi.  This file knows no leaves and no range.  Every operation is float32 or float64
exactly as the header types it (asserted).  Only the gradient term is stated here: the Godunov selection and the step are
sdf_track_ref's expressions, and the trim, the schedule, the dilation and the flows are sdf_track_ref / sdf_grow_ref / sdf_flow_ref
themselves, run with this file's pass in place of the first-order one (hjweno5()).
  weno5()           W5 of five float32 arrays
  axis_diffs()      (dm, dp) of seven float32 arrays u(-3..3)
  voxel_value()     the new value of a voxel from its 19 values (three septuples that share the middle)
  norm_pass_weno()  one normalisation pass
  track()  tracked()  grown()  flow()   sdf_track_ref.track / tracked, sdf_grow_ref.grown, sdf_flow_ref.flow under HJWENO5
  CASES             the (W, K, offset / dx, N, trim) the host and GPU tests share
Pinned: tests/test_vdb_ref.py holds weno5(), axis_diffs(), voxel_value() and norm_pass_weno() bit for bit to OpenVDB's own WENO5, D1 and
Normalizer::eval over the NineteenPointStencil, compiled in place (oracle/vdb_ref.cpp).
"""
import contextlib

import numpy as np

import sdf_flow_ref
import sdf_grow_ref
import sdf_track_ref as T

F, D = np.float32, np.float64
FIRST, HJWENO5 = 0, 4
CASES = [(1, 1, 0.0, 3, 1), (1, 2, -0.25, 3, 1), (1, 0, 0.6, 2, 1), (2, 1, 0.0, 1, 0)]


def _f(x):
    assert x.dtype == F, x.dtype
    return x


def _d(x):
    assert x.dtype == D, x.dtype
    return x


def _sqf(x):
    return _f(_f(x) * x)


def _sqd(x):
    return _d(_d(x) * x)


def weno5(v1, v2, v3, v4, v5):
    v1, v2, v3, v4, v5 = (np.asarray(v, dtype=F) for v in (v1, v2, v3, v4, v5))
    C = D(13.0) / D(12.0)
    eps = D(1.0e-6) * D(F(0.01))
    w = lambda x: _f(x).astype(D)   # noqa: E731
    s1 = _d(_d(C * w(_sqf(_f(_f(v1 - _f(F(2) * v2)) + v3))) + D(0.25) * _sqd(w(_f(v1 - _f(F(4) * v2))) + D(3.0) * w(v3))) + eps)
    s2 = _d(_d(C * w(_sqf(_f(_f(v2 - _f(F(2) * v3)) + v4))) + D(0.25) * w(_sqf(_f(v2 - v4)))) + eps)
    s3 = _d(_d(C * w(_sqf(_f(_f(v3 - _f(F(2) * v4)) + v5))) + D(0.25) * _sqd(_d(D(3.0) * w(v3) - w(_f(F(4) * v4))) + w(v5))) + eps)
    A1, A2, A3 = _d(D(0.1) / (s1 * s1)), _d(D(0.6) / (s2 * s2)), _d(D(0.3) / (s3 * s3))
    d1, d2, d3, d4, d5 = w(v1), w(v2), w(v3), w(v4), w(v5)
    num = _d(_d(A1 * ((D(2.0) * d1 - D(7.0) * d2) + D(11.0) * d3) + A2 * ((D(5.0) * d3 - d2) + D(2.0) * d4)) + A3 * ((D(2.0) * d3 + D(5.0) * d4) - d5))
    return _f(_d(num.astype(F).astype(D) / (D(6.0) * ((A1 + A2) + A3))).astype(F))


def axis_diffs(u):
    """(dm, dp) from u[k + 3] = val(c + k e), k = -3..3 (seven float32 arrays of one shape)."""
    u = [np.asarray(x, dtype=F) for x in u]
    dp = weno5(_f(u[6] - u[5]), _f(u[5] - u[4]), _f(u[4] - u[3]), _f(u[3] - u[2]), _f(u[2] - u[1]))
    dm = _f(-weno5(_f(u[0] - u[1]), _f(u[1] - u[2]), _f(u[2] - u[3]), _f(u[3] - u[4]), _f(u[4] - u[5])))
    return dm, dp


def _step(p, terms, dx):
    """sdf_track_ref.norm_pass's tail: G, S and the new value from the three axis terms (x, y, z)."""
    dx = F(dx)
    dt, inv = _f(dx * F(0.3)), _f(F(1) / dx)
    G = terms[0]
    G = _f(G + terms[1])
    G = _f(G + terms[2])
    S = _f(p / _f(_f(np.sqrt(_f(_f(p * p) + G))) + T.TOL))
    slope = _f(_f(_f(np.sqrt(G)) * inv) - F(1))
    return _f(p - _f(_f(dt * S) * slope))


def _term(out, dm, dp):
    zero = np.zeros_like(dm)
    A = np.where(out, T.fmax(dm, zero), T.fmin(dm, zero))
    B = np.where(out, T.fmin(dp, zero), T.fmax(dp, zero))
    return _f(T.fmax(_f(A * A), _f(B * B)))


def voxel_value(ux, uy, uz, dx):
    """The new value of active voxels from their 19 values: ux, uy, uz are septuples (7, ...) whose middles are the voxel's own."""
    ux, uy, uz = (np.asarray(u, dtype=F) for u in (ux, uy, uz))
    p = ux[3]
    assert np.array_equal(uy[3].view(np.uint32), p.view(np.uint32)) and np.array_equal(uz[3].view(np.uint32), p.view(np.uint32))
    out = p > F(0)
    return _step(p, [_term(out, *axis_diffs(list(u))) for u in (ux, uy, uz)], dx)


def norm_pass_weno(val, act, bg, dx):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    P = np.pad(val, 3, constant_values=F(bg))
    out = val > F(0)
    terms = []
    for a in range(3):
        u = []
        for k in range(-3, 4):
            sl = [slice(3, n + 3)] * 3
            sl[a] = slice(3 + k, 3 + k + n)
            u.append(P[tuple(sl)])
        terms.append(_term(out, *axis_diffs(u)))
    return np.where(act, _step(val, terms, dx), val)


@contextlib.contextmanager
def hjweno5():
    """Inside: every track of sdf_track_ref, sdf_grow_ref and sdf_flow_ref normalises with norm_pass_weno (they all go through
    sdf_track_ref.track, which looks its pass up by name).  Nothing cached by those files is made inside."""
    first = T.norm_pass
    T.norm_pass = norm_pass_weno
    try:
        yield
    finally:
        T.norm_pass = first


def track(val, act, bg, dx, N, do_trim, scheme=HJWENO5):
    if scheme == FIRST:
        return T.track(val, act, bg, dx, N, do_trim)
    with hjweno5():
        return T.track(val, act, bg, dx, N, do_trim)


def tracked(val, act, bg, dx, W, K, offset, N, do_trim):
    with hjweno5():
        return T.tracked(val, act, bg, dx, W, K, offset, N, do_trim)


def grown(val, act, bg, dx, W, K, offset, N, ids=None, vel=None):
    with hjweno5():
        return sdf_grow_ref.grown(val, act, bg, dx, W, K, offset, N, ids, vel)


def flow(kind, val, act, bg, dx, W, K, offset=0.0, N=0, do_trim=False, grow=False, ids=None, vel=None):
    with hjweno5():
        return sdf_flow_ref.flow(kind, val, act, bg, dx, W, K, offset, N, do_trim, grow, ids, vel)


# ---- the sphere of the drift figures: an exact signed distance clamped to the band ------------------------------------------------
SPHERE_N, SPHERE_CENTRE, SPHERE_BG = 32, (15.8, 15.7, 16.0), 3.0
SPHERE_RADII = (4.0, 6.0, 9.0)


def sphere(R, n=SPHERE_N, centre=SPHERE_CENTRE, bg=SPHERE_BG):
    """(val, act, d): the exact distance d (float64) to a sphere of radius R voxels, dx = 1; val = d clamped to +-bg as float32,
    active where |d| < bg."""
    x = np.arange(n, dtype=D)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    d = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - R
    val = np.clip(d, -bg, bg).astype(F)
    return val, np.abs(d) < bg, d


def drift(val, act, d, width=1.5):
    """max |val - d| over the active voxels with |d| < width (float64; a figure, not a definition)."""
    m = act & (np.abs(d) < width)
    assert m.any()
    return float(np.abs(val.astype(D)[m] - d[m]).max())


# ---- the tracked scenes the tests share: computed once per process, never modified -------------------------------------------------
_cache = {}


def scene(name, n, R, w, dx, case):
    """(tracked val, tracked act, bg, mesh_ref.mesh(tracked val)) of a named scene of tests/mesh_ref.py for a case of CASES; cached."""
    import mesh_ref
    import sdf_filter_ref
    key = (name, n, R, w, dx) + tuple(case)
    if key not in _cache:
        _, val, act, bg, _ = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))
        W, K, units, N, tr = case
        vt, at = tracked(val, act, bg, dx, W, K, units * dx, N, bool(tr))
        vt.setflags(write=False)
        at.setflags(write=False)
        _cache[key] = (vt, at, bg, mesh_ref.mesh(vt))
    return _cache[key]
