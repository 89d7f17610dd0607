"""Reference for the grown track of the liquid surface (include/fluid_hip.h, "liquid surface, grown band") — test infrastructure,
numpy only.

OpenVDB's LevelSetTracker::track() in full (tools/LevelSetTracker.h:293-306): dilateActiveValues(1, NN_FACE), normalize(), Trim,
on a dense (val, act) (n, n, n) of tests/sdf_ref.py closed().  The dilation is clipped by the grid and by nothing else: this file
knows no leaves and no range.  Built on sdf_track_ref (norm_pass, trim, offset_steps) and sdf_filter_ref (box_pass); every value
is float32 (asserted in those files and here).
  dilate()        one dilation of the mask: a voxel or one of its six face neighbours was active
  dilate_attr()   the same with ids and velocities: a new voxel takes the first active neighbour's in the order -x +x -y +y -z +z
  grown_track()   one dilation, N normalisation passes, the trim; grow=False is sdf_track_ref.track with the trim
  grown()         the tracked filter (W, K, offset; N) with every track a grown one; with ids / vel the attribute form
  GROWS           the (W, K, offset / dx, N) the host and GPU tests share, all with the trim
Pinned: the passes this file composes (sdf_track_ref, sdf_filter_ref) are held to OpenVDB's own lines by tests/test_vdb_ref.py; the
dilation (tools/Morphology.h) is still this file's reading alone.
"""
import numpy as np

import sdf_filter_ref
import sdf_track_ref

F = np.float32
NO_ID = np.uint32(0xFFFFFFFF)
GROWS = [(1, 0, -3.0, 3), (1, 1, -3.0, 3), (1, 0, -1.0, 3), (1, 1, 0.0, 3), (1, 0, 1.0, 3), (2, 2, -4.0, 2), (1, 0, -0.25, 1)]
BLOCK_GROWS = [(1, 0, 1.0, 3), (1, 0, 2.0, 3), (1, 0, 3.0, 3)]          # the 13^3 block: the band walks inwards through -bg
ORDER6 = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))            # (axis, step): -x +x -y +y -z +z


def _shifted(a, axis, step, fill):
    """b with b[c] = a[c + step e_axis], `fill` where that lies outside the grid."""
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (1, 1)
    P = np.pad(a, pad, constant_values=fill)
    sl = [slice(None)] * a.ndim
    sl[axis] = slice(1 + step, 1 + step + n)
    return P[tuple(sl)]


def dilate(act):
    act = np.asarray(act, dtype=bool)
    out = act.copy()
    for axis, step in ORDER6:
        out |= _shifted(act, axis, step, False)
    return out


def dilate_attr(act, ids, vel):
    """(act_new, ids_new, vel_new); ids (n, n, n) uint32, vel (3, n, n, n) float32.  Reads everything as it was before."""
    act = np.asarray(act, dtype=bool)
    new, ids2, vel2 = act.copy(), np.array(ids, dtype=np.uint32), np.array(vel, dtype=F)
    for axis, step in ORDER6:
        take = _shifted(act, axis, step, False) & ~new          # not active before, and no earlier neighbour gave
        ids2 = np.where(take, _shifted(ids, axis, step, NO_ID), ids2)
        for a in range(3):
            vel2[a] = np.where(take, _shifted(vel[a], axis, step, F(0)), vel2[a])
        new |= take
    assert ids2.dtype == np.uint32 and vel2.dtype == F
    return new, ids2, vel2


def grown_track(val, act, bg, dx, N, ids=None, vel=None, grow=True):
    assert N >= 1
    attr = ids is not None
    if grow:
        if attr:
            act, ids, vel = dilate_attr(act, ids, vel)
        else:
            act = dilate(act)
    before = act
    val, act = sdf_track_ref.track(val, act, bg, dx, N, True)
    assert val.dtype == F
    if attr:
        gone = before & ~act
        ids = np.where(gone, NO_ID, ids).astype(np.uint32)
        vel = np.where(gone[None], F(0), vel).astype(F)
        return val, act, ids, vel
    return val, act


def grown(val, act, bg, dx, W, K, offset, N, ids=None, vel=None, grow=True):
    """(val, act[, ids, vel]) after the tracked filter whose every track is a grown one; offset in world units."""
    val, act = np.array(val, dtype=F), np.array(act, dtype=bool)
    attr = ids is not None
    if grow:
        assert abs(F(offset)) <= F(4) * F(dx)
    st = (val, act, ids, vel) if attr else (val, act)
    for _ in range(K):
        v = st[0]
        for a in sdf_filter_ref.ORDER:
            v = sdf_filter_ref.box_pass(v, st[1], bg, W, a)
        st = grown_track(v, st[1], bg, dx, N, *st[2:], grow=grow)
    for step in sdf_track_ref.offset_steps(offset, dx):
        v = np.where(st[1], st[0] + step, st[0])
        assert v.dtype == F
        st = grown_track(v, st[1], bg, dx, N, *st[2:], grow=grow)
    return st


def tracks(K, offset, dx):
    """T: how many tracks the filter runs."""
    return K + len(sdf_track_ref.offset_steps(offset, dx))


def positions(name, n):
    import mesh_ref
    if name == "faces":                                                      # one leaf unfiltered; grows through all six faces
        return np.array([[3.5, 3.5, 3.5]])
    if name == "block":                                                      # 13^3 particles at the integer points -6..6
        r = np.arange(-6.0, 7.0)
        return np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    return mesh_ref.positions(name, n)


# ---- the grown scenes the tests share: computed once per process, never modified -------------------------------------------------
_base, _cache = {}, {}


def base(name, n, R, w, dx):
    """(pos, vel, val, act, ids, vel32, bg) of the unfiltered scene; cached."""
    import attr_ref
    import sdf_ref
    key = (name, n, R, w, dx)
    if key not in _base:
        pos = positions(name, n)
        vel = attr_ref.velocities(pos)
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        ids, v32 = attr_ref.closest(pos, vel, n, R, w, dx)
        for a in (pos, vel, val, act, ids, v32):
            a.setflags(write=False)
        _base[key] = (pos, vel, val, act, ids, v32, sdf_ref.constants(R, w, dx)[3])
    return _base[key]


def scene(name, n, R, w, dx, case):
    """(val, act, ids, vel32) of a scene after the grown filter of a case (W, K, offset / dx, N); cached."""
    key = (name, n, R, w, dx) + tuple(case)
    if key not in _cache:
        _, _, val, act, ids, v32, bg = base(name, n, R, w, dx)
        W, K, units, N = case
        out = grown(val, act, bg, dx, W, K, units * dx, N, ids, v32)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
