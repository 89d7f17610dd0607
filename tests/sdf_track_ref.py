"""Reference for the renormalised liquid surface (include/fluid_hip.h, "liquid surface, renormalised") — test infrastructure,
numpy only.

OpenVDB's LevelSetTracker::normalize() with FIRST_BIAS / TVD_RK1 and Trim (tools/LevelSetTracker.h:293-306, 455-475, 485-494,
596-609; math/Operators.h:252-284; math/FiniteDifference.h:352-374; math/Math.h:118) without the band dilation, and the stepped
offset of tools/LevelSetFilter.h:352-368, on a dense (val, act) (n, n, n) of tests/sdf_ref.py closed(): the grid is padded with
+bg, every operation is a float32 operation (asserted), max and min are explicit np.where, a pass is Jacobi.
  norm_pass()  one normalisation pass; `axes` and `assoc` are parameters only so that a test can show that they matter
  trim()       the trim
  track()      N passes, then the trim
  tracked()    the tracked filter (W, K, offset; N, trim); N = 0 without trim is sdf_filter_ref.smooth()
  TRACKS       the (W, K, offset / dx, N, trim) the host and GPU tests share
Pinned: tests/test_vdb_ref.py holds norm_pass() and offset_steps() bit for bit to OpenVDB's own Normalizer::eval and offset(), compiled in
place (oracle/vdb_ref.cpp); trim() is restated there in three lines from tools/LevelSetTracker.h:469-472.
"""
import numpy as np

import sdf_filter_ref

F = np.float32
TOL = F(1e-8)
TRACKS = [(1, 1, 0.0, 3, 1), (1, 2, 0.0, 3, 1), (2, 1, 0.0, 1, 0), (1, 0, -0.25, 3, 1), (1, 0, 0.6, 2, 1), (4, 3, 0.0, 2, 1),
          (1, 1, 0.0, 0, 0)]


def fmax(a, b):
    return np.where(a < b, b, a)


def fmin(a, b):
    return np.where(b < a, b, a)


def _f(x):
    assert x.dtype == F, x.dtype
    return x


def norm_pass(val, act, bg, dx, axes=(0, 1, 2), assoc=False):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    dx = F(dx)
    dt, inv = _f(dx * F(0.3)), _f(F(1) / dx)
    P = np.pad(val, 1, constant_values=F(bg))
    p = val
    out = p > F(0)
    zero = np.zeros_like(p)
    t = []
    for a in range(3):
        lo, hi = [slice(1, n + 1)] * 3, [slice(1, n + 1)] * 3
        lo[a], hi[a] = slice(0, n), slice(2, n + 2)
        dm, dp = _f(p - P[tuple(lo)]), _f(P[tuple(hi)] - p)
        A = np.where(out, fmax(dm, zero), fmin(dm, zero))
        B = np.where(out, fmin(dp, zero), fmax(dp, zero))
        t.append(_f(fmax(_f(A * A), _f(B * B))))
    G = t[axes[0]]
    G = _f(G + t[axes[1]])
    G = _f(G + t[axes[2]])
    S = _f(p / _f(_f(np.sqrt(_f(_f(p * p) + G))) + TOL))
    slope = _f(_f(_f(np.sqrt(G)) * inv) - F(1))
    v = _f(p - (_f(dt * _f(S * slope)) if assoc else _f(_f(dt * S) * slope)))
    return np.where(act, v, val)


def trim(val, act, bg):
    bg = F(bg)
    neg, pos = act & (val <= -bg), act & (val >= bg)
    val = np.where(neg, -bg, np.where(pos, bg, val))
    return _f(val), act & ~neg & ~pos


def track(val, act, bg, dx, N, do_trim):
    for _ in range(N):
        val = norm_pass(val, act, bg, dx)
    if do_trim:
        val, act = trim(val, act, bg)
    return val, act


def offset_steps(offset, dx):
    """The signed steps of a tracked offset, float32."""
    off, dx = F(offset), F(dx)
    cfl = _f(F(0.5) * dx)
    a, d = np.abs(off), F(0)
    out = []
    while _f(a - d) > _f(F(0.001) * cfl):
        delta = _f(a - d) if _f(a - d) < cfl else cfl
        d = _f(d + delta)
        out.append(np.copysign(delta, off))
    return out


def tracked(val, act, bg, dx, W, K, offset, N, do_trim):
    """(val, act) after the tracked filter; offset in world units, as the C interface takes it."""
    if N == 0 and not do_trim:
        return sdf_filter_ref.smooth(val, act, bg, W, K, offset), np.array(act)
    val, act = np.array(val, dtype=F), np.array(act)
    assert abs(F(offset)) <= F(bg)
    for _ in range(K):
        for a in sdf_filter_ref.ORDER:
            val = sdf_filter_ref.box_pass(val, act, bg, W, a)
        val, act = track(val, act, bg, dx, N, do_trim)
    for step in offset_steps(offset, dx):
        val = np.where(act, _f(val + step), val)
        val, act = track(val, act, bg, dx, N, do_trim)
    return val, act


def gradient_error(val, act, bg, dx):
    """Mean central-difference | |grad val| - 1 | over the active voxels with |val| < bg / 2 (double; a figure, not a definition)."""
    P = np.pad(np.asarray(val, dtype=np.float64), 1, constant_values=float(bg))
    n = val.shape[0]
    g2 = np.zeros(val.shape)
    for a in range(3):
        lo, hi = [slice(1, n + 1)] * 3, [slice(1, n + 1)] * 3
        lo[a], hi[a] = slice(0, n), slice(2, n + 2)
        g2 += ((P[tuple(hi)] - P[tuple(lo)]) / (2.0 * float(dx))) ** 2
    m = act & (np.abs(val) < float(bg) / 2)
    return float(np.abs(np.sqrt(g2[m]) - 1.0).mean())


# ---- the tracked scenes the tests share: computed once per process, never modified -----------------------------------------------
_cache = {}


def scene(name, n, R, w, dx, case):
    """(positions, tracked val, tracked act, bg, mesh_ref.mesh(tracked val)) of a named scene of tests/mesh_ref.py for a case
    (W, K, offset / dx, N, trim) of TRACKS; cached."""
    import mesh_ref
    key = (name, n, R, w, dx) + tuple(case)
    if key not in _cache:
        pos, val, act, bg, _ = sdf_filter_ref.scene(name, n, R, w, dx, (1, 0, 0.0))
        W, K, units, N, tr = case
        vt, at = tracked(val, act, bg, dx, W, K, units * dx, N, bool(tr))
        vt.setflags(write=False)
        at.setflags(write=False)
        _cache[key] = (pos, vt, at, bg, mesh_ref.mesh(vt))
    return _cache[key]
