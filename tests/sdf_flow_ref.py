"""Reference for the flows of the liquid surface (include/fluid_hip.h, "liquid surface, flows") — test infrastructure, numpy only.

The median, Laplacian and mean-curvature filters of OpenVDB's LevelSetFilter (tools/LevelSetFilter.h:256-268, 318-347, 380-409,
421-450, 481-507; math/Stencils.h:147-155, 1230-1238, 1283-1288, 1506-1540, 1596-1619, 1670-1680) on a dense (val, act) (n, n, n)
of tests/sdf_ref.py closed(): the grid is padded with +bg, a pass is Jacobi, only active voxels change.  This file knows no leaves
and no range.  The Laplacian is float32 throughout (asserted); the curvature term is formed in float64 from float32 differences
and narrowed once; the median is np.partition over the monotone uint32 keys of the values' bytes.  Composes with sdf_filter_ref
(box passes), sdf_track_ref (track, offset steps) and sdf_grow_ref (dilation, attributes).
  consts()          inv2dx, invdx2 and the two time steps
  laplacian_pass()  curvature_pass()  median_pass()  one pass each;  flow_pass() by kind
  keys() / unkeys() the median's order
  flow()            the filter of a kind: K iterations, tracks, the offset; untracked, tracked or grown; with ids / vel the attributes
  CASES             the (kind, W) the host and GPU tests share
Pinned: tests/test_vdb_ref.py holds consts() and the three passes bit for bit to OpenVDB's own GradStencil, CurvatureStencil and
DenseStencil::median and the filter's two time steps, compiled in place (oracle/vdb_ref.cpp), on inputs without -0.0: between
signed zeros keys() is this project's own order.
"""
import numpy as np

import sdf_filter_ref
import sdf_grow_ref as G
import sdf_track_ref as T

F, D = np.float32, np.float64
BOX, MEDIAN, LAPLACIAN, CURVATURE = 0, 1, 2, 3
CASES = [(LAPLACIAN, 1), (CURVATURE, 1), (MEDIAN, 1), (MEDIAN, 2)]
NAMES = {BOX: "box", MEDIAN: "median", LAPLACIAN: "laplacian", CURVATURE: "curvature"}


def _f(x):
    assert x.dtype == F, x.dtype
    return x


def _d(x):
    assert x.dtype == D, x.dtype
    return x


def consts(dx):
    """(invdx2, dt_laplacian, dt_curvature), float32."""
    dx = F(dx)
    inv2dx = F(D(0.5) / D(dx))
    invdx2 = F(D(4.0) * D(inv2dx) * D(inv2dx))
    return invdx2, F(F(dx * dx) / F(6)), F(F(dx * dx) / F(3))


def _view(P, n, H, i, j, k):
    """val(c + (i, j, k)) for every c of the grid, from the grid padded by H."""
    return P[H + i:H + i + n, H + j:H + j + n, H + k:H + k + n]


def laplacian_pass(val, act, bg, dx):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    invdx2, dt, _ = consts(dx)
    P = np.pad(val, 1, constant_values=F(bg))
    v = lambda i, j, k: _view(P, n, 1, i, j, k)   # noqa: E731
    s = _f(v(-1, 0, 0) + v(1, 0, 0))
    for nb in ((0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
        s = _f(s + v(*nb))
    L = _f(invdx2 * _f(s - _f(F(6) * val)))
    return np.where(act, _f(val + _f(dt * L)), val)


def curvature_pass(val, act, bg, dx):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    invdx2, _, dt = consts(dx)
    P = np.pad(val, 1, constant_values=F(bg))
    v = lambda i, j, k: _view(P, n, 1, i, j, k)   # noqa: E731
    p = val
    xm, xp, ym, yp, zm, zp = v(-1, 0, 0), v(1, 0, 0), v(0, -1, 0), v(0, 1, 0), v(0, 0, -1), v(0, 0, 1)
    Dx, Dy, Dz = (_d(D(0.5) * _f(b - a).astype(D)) for a, b in ((xm, xp), (ym, yp), (zm, zp)))
    Dx2, Dy2, Dz2 = Dx * Dx, Dy * Dy, Dz * Dz
    ng = _d((Dx2 + Dy2) + Dz2)
    Dxx, Dyy, Dzz = (_f(_f(b - _f(F(2) * p)) + a).astype(D) for a, b in ((xm, xp), (ym, yp), (zm, zp)))

    def mixed(a, b, c, d):
        return _d(D(0.25) * _f(_f(_f(v(*a) - v(*b)) + v(*c)) - v(*d)).astype(D))

    Dxy = mixed((1, 1, 0), (1, -1, 0), (-1, -1, 0), (-1, 1, 0))
    Dxz = mixed((1, 0, 1), (1, 0, -1), (-1, 0, -1), (-1, 0, 1))
    Dyz = mixed((0, 1, 1), (0, 1, -1), (0, -1, -1), (0, -1, 1))
    alpha = _d(((Dx2 * (Dyy + Dzz) + Dy2 * (Dxx + Dzz)) + Dz2 * (Dxx + Dyy)) - D(2.0) * ((Dx * ((Dy * Dxy) + (Dz * Dxz))) + ((Dy * Dz) * Dyz)))
    flat = ng <= D(1e-15)
    beta = np.sqrt(np.where(flat, D(1), ng))
    term = _d((alpha * D(invdx2)) / (D(2.0) * (beta * beta)))
    Fv = np.where(flat, F(0), term.astype(F))
    return np.where(act, _f(p + _f(dt * _f(Fv))), val)


def keys(val):
    """The monotone uint32 key of every float32's bytes: -0 sorts before +0, equal keys are equal bytes."""
    b = np.ascontiguousarray(val, dtype=F).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F)


def median_of(values):
    """The element at rank (m - 1) >> 1 of a 1-d float32 array, in the key order."""
    k = keys(np.asarray(values, dtype=F).ravel())
    r = (len(k) - 1) >> 1
    return unkeys(np.partition(k, r)[r:r + 1])[0]


def median_pass(val, act, bg, W):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    assert not np.isnan(val).any()
    P = keys(np.pad(val, W, constant_values=F(bg)))
    r = range(-W, W + 1)
    cube = np.stack([_view(P, n, W, i, j, k) for i in r for j in r for k in r])
    rank = (len(cube) - 1) >> 1
    med = unkeys(np.partition(cube, rank, axis=0)[rank])
    return np.where(act, med, val)


def flow_pass(kind, val, act, bg, dx, W):
    if kind == MEDIAN:
        assert W in (1, 2)
        return median_pass(val, act, bg, W)
    assert W == 1
    return laplacian_pass(val, act, bg, dx) if kind == LAPLACIAN else curvature_pass(val, act, bg, dx)


def iteration(kind, val, act, bg, dx, W):
    """One iteration: the box filter's three passes, or the one pass of a flow."""
    if kind == BOX:
        for a in sdf_filter_ref.ORDER:
            val = sdf_filter_ref.box_pass(val, act, bg, W, a)
        return val
    return flow_pass(kind, val, act, bg, dx, W)


def _track(val, act, bg, dx, N, do_trim, grow, ids, vel):
    if grow:
        if ids is not None:
            act, ids, vel = G.dilate_attr(act, ids, vel)
        else:
            act = G.dilate(act)
    before = act
    val, act = T.track(val, act, bg, dx, N, do_trim)
    if ids is not None:
        gone = before & ~act
        ids = np.where(gone, G.NO_ID, ids).astype(np.uint32)
        vel = np.where(gone[None], F(0), vel).astype(F)
    return val, act, ids, vel


def flow(kind, val, act, bg, dx, W, K, offset=0.0, N=0, do_trim=False, grow=False, ids=None, vel=None):
    """(val, act, ids, vel) after the filter of `kind`; offset in world units; ids / vel None without attributes.  N = 0 without
    trim: untracked (the offset in one step); grow needs N >= 1 and the trim."""
    val, act = np.array(val, dtype=F), np.array(act, dtype=bool)
    tracked = N > 0 or do_trim
    assert not grow or (N >= 1 and do_trim)
    for _ in range(K):
        val = iteration(kind, val, act, bg, dx, W)
        if tracked:
            val, act, ids, vel = _track(val, act, bg, dx, N, do_trim, grow, ids, vel)
    if tracked:
        for step in T.offset_steps(offset, dx):
            val = np.where(act, _f(val + step), val)
            val, act, ids, vel = _track(val, act, bg, dx, N, do_trim, grow, ids, vel)
    elif F(offset) != F(0):
        val = np.where(act, _f(val + F(offset)), val)
    return _f(val), act, ids, vel


# ---- the scenes the tests share: computed once per process, never modified ---------------------------------------------------------
SCENES = [("one", 16), ("corner", 16), ("lo", 16), ("hi", 16), ("cloud", 16), ("one", 25), ("corner", 25), ("lo", 25), ("hi", 25), ("cloud", 25),
          ("leafcorner", 32)]
_base, _cache = {}, {}


def positions(name, n):
    if name == "leafcorner":   # base cell (0, 0, 0): the min-corner voxel of the leaf at the origin, whose 26 neighbours the n = 32 grid holds
        return np.array([[0.2, 0.1, 0.3]])
    return G.positions(name, n)


def base(name, n, R, w, dx):
    """(pos, val, act, ids, vel32, bg) of the unfiltered scene; cached."""
    import attr_ref
    import sdf_ref
    key = (name, n, R, w, dx)
    if key not in _base:
        pos = positions(name, n)
        vel = attr_ref.velocities(pos)
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        ids, v32 = attr_ref.closest(pos, vel, n, R, w, dx)
        for a in (pos, val, act, ids, v32):
            a.setflags(write=False)
        _base[key] = (pos, val, act, ids, v32, sdf_ref.constants(R, w, dx)[3])
    return _base[key]


def scene(name, n, R, w, dx, kind, W, K, units, N, do_trim, grow):
    """(val, act, ids, vel32) of a scene after flow(kind, ...) with offset = units * dx; cached."""
    key = (name, n, R, w, dx, kind, W, K, units, N, do_trim, grow)
    if key not in _cache:
        _, val, act, ids, v32, bg = base(name, n, R, w, dx)
        out = flow(kind, val, act, bg, dx, W, K, units * dx, N, do_trim, grow, ids, v32)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
