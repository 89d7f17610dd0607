"""Reference for the liquid surface's attributes (include/fluid_hip.h, "liquid surface, attributes") — test infrastructure, numpy only.

Per active voxel the id and the narrowed velocity of the closest counted particle — the smallest id among the particles whose
x2y2z2 equals the voxel's minimum —, per mesh vertex a velocity interpolated along the counting edges:
  closest()          ids (n, n, n) uint32 and velocities (3, n, n, n) float32 as a closed form over the particle set;
  sequential()       the loop of sdf_ref.sequential restated particle by particle, carrying (m, id), in any visiting order;
  vertex_velocity()  (nv, 3) float32 in mesh_ref.mesh's vertex order, and how many counting edges had two, one or no active end;
  leaf_attr()        the attributes of sdf_ref.leaf_list's leaves: ids (k, 512), velocities (k, 3, 512).
"""
import numpy as np

import sdf_ref
from mesh_ref import _order
from sdf_ref import F, geometry

NO_ID = np.uint32(0xFFFFFFFF)


def _mask(idg, act, vel):
    """NO_ID / +0 where the voxel is not active, the winner's id and narrowed velocity elsewhere."""
    ids = np.where(act, idg, np.int64(NO_ID)).astype(np.uint32)
    v32 = np.asarray(vel, dtype=np.float64).reshape(-1, 3).astype(F)           # one narrowing, no scaling
    out = np.zeros((3,) + act.shape, dtype=F)
    for a in range(3):
        out[a][act] = v32[ids[act], a]
    return ids, out


def closest(pos, vel, n, R, w, dx):
    """(id (n, n, n) uint32, vel (3, n, n, n) float32); a particle's id is its row in pos."""
    lo, hi, _, _ = geometry(n)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    reach = int(np.ceil(float(F(F(R) + F(w))))) + 1
    m = sdf_ref.min_dist2(pos, n, reach).ravel()
    _, act = sdf_ref.closed(pos, n, R, w, dx)
    c = sdf_ref.base_cell(pos)
    rows = np.flatnonzero(((c >= lo) & (c <= hi)).all(axis=1))                  # the counted particles, by id
    P, c = pos[rows], c[rows]
    idg = np.full(n * n * n, np.int64(NO_ID), dtype=np.int64)
    r = np.arange(-reach, reach + 1)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    step = max(1, 2_000_000 // len(off))
    for s in range(0, len(P), step):
        v = c[s:s + step, None, :] + off[None, :, :]
        ok = ((v >= lo) & (v <= hi)).all(axis=2)
        d = sdf_ref.dist2(v[..., 0], v[..., 1], v[..., 2], P[s:s + step, None, :])
        idx = ((v[..., 0] - lo) * n + (v[..., 1] - lo)) * n + (v[..., 2] - lo)
        idx = np.where(ok, idx, 0)
        hit = ok & (d == m[idx])                                               # the particles AT the voxel's minimum
        pid = np.broadcast_to(rows[s:s + step, None], idx.shape)
        np.minimum.at(idg, idx[hit], pid[hit])                                 # ... and the smallest id among them
    return _mask(idg.reshape(n, n, n), act, vel)


def sequential(pos, vel, n, R, w, dx, order=None):
    """The rasteriser's loop, one particle after the other in `order` (default: as given), carrying the minimum and who gave it."""
    lo, hi, _, _ = geometry(n)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    mx = float(F(F(R) + F(w)))
    m = np.full((n, n, n), np.inf, dtype=F)
    idg = np.full((n, n, n), np.int64(NO_ID), dtype=np.int64)
    c = sdf_ref.base_cell(pos)
    counted = ((c >= lo) & (c <= hi)).all(axis=1)
    for i in (range(len(pos)) if order is None else order):
        if not counted[i]:
            continue
        p = pos[i]
        a = np.maximum(np.floor(p - mx).astype(int), lo)
        b = np.minimum(np.ceil(p + mx).astype(int), hi)
        if (a > b).any():
            continue
        gx, gy, gz = np.meshgrid(*[np.arange(a[k], b[k] + 1) for k in range(3)], indexing="ij")
        d2 = sdf_ref.dist2(gx, gy, gz, p)
        sl = tuple(slice(a[k] - lo, b[k] - lo + 1) for k in range(3))
        mm, ii = m[sl], idg[sl]                                                # views
        less = d2 < mm
        tie = (d2 == mm) & (i < ii)
        ii[less | tie] = i
        mm[less] = d2[less]
    _, act = sdf_ref.closed(pos, n, R, w, dx)                                  # (equal to sdf_ref.sequential: tests/test_sdf_ref.py)
    return _mask(idg, act, vel)


def vertex_velocity(val, act, vel):
    """((nv, 3) float32 in mesh_ref.mesh(val)'s vertex order, {"two", "one", "none"}: counting edges by active ends, and
    {"vertices", "empty", "partial"}: vertices, those with kv == 0 and those with 0 < kv < k)."""
    val = np.ascontiguousarray(val, dtype=F)
    act = np.asarray(act, dtype=bool)
    n = val.shape[0]
    lo, _, _, _ = geometry(n)
    m = n - 1

    def corner(a, d):
        return a[..., d[0]:d[0] + m, d[1]:d[1] + m, d[2]:d[2] + m]
    inside = val < F(0)
    cnt = np.zeros((m, m, m), int)
    for d in np.ndindex(2, 2, 2):
        cnt += corner(inside, d)
    mixed = (cnt > 0) & (cnt < 8)
    s = np.zeros((3, m, m, m), F)
    kv = np.zeros((m, m, m), int)
    kc = np.zeros((m, m, m), int)                                               # counting edges, contributing or not
    classes = {"two": 0, "one": 0, "none": 0}
    zero = F(0)
    for a in range(3):
        b1, b2 = [x for x in range(3) if x != a]
        for d1, d2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            d0 = [0, 0, 0]
            d0[b1], d0[b2] = d1, d2
            e1 = list(d0)
            e1[a] = 1
            v0, v1 = corner(val, d0), corner(val, e1)
            A0, A1 = corner(act, d0), corner(act, e1)
            counts = (v0 < zero) != (v1 < zero)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = v0 / (v0 - v1)
            both, one, none = counts & A0 & A1, counts & (A0 ^ A1), counts & ~A0 & ~A1
            classes["two"] += int(both.sum())
            classes["one"] += int(one.sum())
            classes["none"] += int(none.sum())
            for x in range(3):
                a0, a1 = corner(vel[x], d0), corner(vel[x], e1)
                with np.errstate(invalid="ignore"):
                    lerp = a0 + t * (a1 - a0)
                assert lerp.dtype == F
                e = np.where(both, lerp, np.where(A0, a0, a1))
                s[x] = s[x] + np.where(both | one, e, zero)
            kv += both | one
            kc += counts
    ci = np.argwhere(mixed)
    ci = ci[_order(ci + lo)]
    k = kv[ci[:, 0], ci[:, 1], ci[:, 2]]
    kf = np.maximum(k, 1).astype(F)
    out = np.stack([np.where(k > 0, s[x][ci[:, 0], ci[:, 1], ci[:, 2]] / kf, zero) for x in range(3)], axis=1).astype(F)
    kall = kc[ci[:, 0], ci[:, 1], ci[:, 2]]
    classes["vertices"] = len(ci)
    classes["empty"] = int((k == 0).sum())                                      # vertices no edge contributes to: +0
    classes["partial"] = int(((k > 0) & (k < kall)).sum())                      # ... and those only some of their edges do
    return out, classes


def leaf_attr(ids, vel, org):
    """ids (k, 512) uint32 and velocities (k, 3, 512) float32 of the leaves with origins org (k, 3): NO_ID / +0 outside the grid."""
    n = ids.shape[0]
    lo, hi, l0, nl = geometry(n)
    pad = nl * 8
    o = lo - l0
    I = np.full((pad,) * 3, NO_ID, dtype=np.uint32)
    V = np.zeros((3,) + (pad,) * 3, dtype=F)
    I[o:o + n, o:o + n, o:o + n] = ids
    V[:, o:o + n, o:o + n, o:o + n] = vel
    oi, ov = np.empty((len(org), 512), np.uint32), np.empty((len(org), 3, 512), F)
    for k, g in enumerate(np.asarray(org) - l0):
        sl = tuple(slice(g[a], g[a] + 8) for a in range(3))
        oi[k] = I[sl].reshape(512)
        ov[k] = V[(slice(None),) + sl].reshape(3, 512)
    return oi, ov


def velocities(pos, seed=7):
    """A non-trivial velocity per particle: double values that do not survive the narrowing unchanged."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, (len(pos), 3)) + 1e-9


def tie_scene():
    """Two particles mirrored in the plane x = 0: every voxel of that plane is exactly as far from one as from the other."""
    pos = np.array([[-0.25, 0.1, 0.2], [0.25, 0.1, 0.2]])
    vel = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.125]])
    return pos, vel


# ---- the scenes the attribute tests share: computed once per process, never modified ---------------------------------------------
_cache = {}


def scene(name, n, R, w, dx, filt=None):
    """(pos, vel, val, act, ids, vel32, (vertex velocity, classes), mesh) of a scene of tests/mesh_ref.py ("tie": tie_scene), with
    velocities(); val is filtered by `filt` = (W, K, offset) when given.  Cached."""
    import mesh_ref
    import sdf_filter_ref
    base = (name, n, R, w, dx)
    if base not in _cache:
        if name == "tie":
            pos, vel = tie_scene()
        else:
            pos = mesh_ref.positions(name, n)
            vel = velocities(pos)
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        ids, v32 = closest(pos, vel, n, R, w, dx)
        for a in (pos, vel, val, act, ids, v32):
            a.setflags(write=False)
        _cache[base] = (pos, vel, val, act, ids, v32)
    key = base + (None if filt is None else tuple(filt),)
    if key not in _cache:
        pos, vel, val, act, ids, v32 = _cache[base]
        vf = val if filt is None else sdf_filter_ref.smooth(val, act, sdf_ref.constants(R, w, dx)[3], *filt)
        vf.setflags(write=False)
        _cache[key] = (pos, vel, vf, act, ids, v32, vertex_velocity(vf, act, v32), mesh_ref.mesh(vf))
    return _cache[key]
