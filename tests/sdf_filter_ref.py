"""Reference for the smoothed liquid surface (include/fluid_hip.h, "liquid surface, smoothed") — test infrastructure, numpy only.

The box filter and offset of OpenVDB's LevelSetFilter (tools/LevelSetFilter.h:213-222, 303-310, 471, 530-535) without the
tracker, on a dense (val, act) (n, n, n) of tests/sdf_ref.py closed(): the grid is padded with +bg (what the library's accessor
returns outside the tree), every add is a float32 add, in ascending order from 0.0f, the sum is multiplied by
frac = float32(1) / float32(2W + 1), an iteration is the axes 0, 2, 1, inactive voxels keep their value, and the offset is added
to the active voxels after the last iteration unless float32(offset) == 0.
  box_pass()  one pass along one axis
  smooth()    K iterations and the offset; `order` is a parameter only so that a test can show that it matters
  FILTERS     the (width, iterations, offset) the host and GPU tests share
Pinned: tests/test_vdb_ref.py holds box_pass() and ORDER bit for bit to OpenVDB's own Avg and box(), compiled in place (oracle/vdb_ref.cpp).
"""
import numpy as np

F = np.float32
ORDER = (0, 2, 1)
FILTERS = [(1, 1, 0.0), (1, 2, 0.0), (2, 1, 0.0), (4, 3, 0.0), (1, 0, -0.25), (3, 2, 0.5), (1, 0, 0.0)]


def box_pass(val, act, bg, W, axis):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (W, W)
    P = np.pad(val, pad, constant_values=F(bg))
    s = np.zeros(val.shape, dtype=F)
    for i in range(2 * W + 1):                                   # i - W = -W .. +W, ascending
        sl = [slice(None)] * 3
        sl[axis] = slice(i, i + n)
        s = s + P[tuple(sl)]
        assert s.dtype == F
    frac = F(1) / F(2 * W + 1)
    out = s * frac
    assert out.dtype == F
    return np.where(act, out, val)


def smooth(val, act, bg, W, K, offset=0.0, order=ORDER):
    """The filtered values (n, n, n) float32; act is unchanged by definition."""
    val = np.array(val, dtype=F)
    for _ in range(K):
        for a in order:
            val = box_pass(val, act, bg, W, a)
    off = F(offset)
    if off != F(0):
        val = np.where(act, val + off, val)
        assert val.dtype == F
    return val


# ---- the filtered scenes the tests share: computed once per process, never modified ---------------------------------------------
_closed, _cache = {}, {}


def scene(name, n, R, w, dx, filt):
    """(positions, filtered val, act, bg, mesh_ref.mesh(filtered val)) of a named scene of tests/mesh_ref.py; cached."""
    import mesh_ref
    import sdf_ref
    base = (name, n, R, w, dx)
    if base not in _closed:
        pos = mesh_ref.positions(name, n)
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        for a in (pos, val, act):
            a.setflags(write=False)
        _closed[base] = (pos, val, act, sdf_ref.constants(R, w, dx)[3])
    key = base + tuple(filt)
    if key not in _cache:
        pos, val, act, bg = _closed[base]
        vf = smooth(val, act, bg, *filt)
        vf.setflags(write=False)
        _cache[key] = (pos, vf, act, bg, mesh_ref.mesh(vf))
    return _cache[key]
