"""Reference for the rank records of the liquid surface's attributes and their merge (include/fluid_hip.h, "liquid surface,
attributes (decomposed runs)") — test infrastructure, numpy only.

  rank_record()  what a rank that holds the particles (pos, vel) with the global ids `ids` lists: origins, values, masks, ids,
                 narrowed velocities and dist2 per leaf.  The subset is sorted by id before attr_ref.closest / sdf_ref.min_dist2
                 see it, so that their "smallest row" is "smallest id"; rows are mapped back to ids afterwards.
  merged()       the attributes of the union: attr_ref.closest over all particles sorted by id, on the union's leaf list.
"""
import numpy as np

import attr_ref
import sdf_ref
from sdf_ref import F

NO_ID = attr_ref.NO_ID


def _by_id(pos, vel, ids):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    ids = np.asarray(ids, dtype=np.uint32).reshape(-1)
    assert len(pos) == len(vel) == len(ids) and len(np.unique(ids)) == len(ids)
    o = np.argsort(ids)
    return pos[o], vel[o], ids[o]


def _leaf_scalar(a, org, fill):
    """(k, 512) of a dense (n, n, n) array for the leaves at org; `fill` outside the grid."""
    n = a.shape[0]
    lo, _, l0, nl = sdf_ref.geometry(n)
    pad, o = nl * 8, lo - l0
    A = np.full((pad,) * 3, fill, dtype=a.dtype)
    A[o:o + n, o:o + n, o:o + n] = a
    out = np.empty((len(org), 512), a.dtype)
    for k, g in enumerate(np.asarray(org).reshape(-1, 3) - l0):
        out[k] = A[g[0]:g[0] + 8, g[1]:g[1] + 8, g[2]:g[2] + 8].reshape(512)
    return out


def _dense(pos, vel, ids, n, R, w, dx):
    """(val, act, global ids, vel32, dist2) on the dense grid for the particles sorted by id."""
    pos, vel, ids = _by_id(pos, vel, ids)
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    rows, v32 = attr_ref.closest(pos, vel, n, R, w, dx)
    gid = np.full(rows.shape, NO_ID, dtype=np.uint32)
    gid[act] = ids[rows[act]]
    reach = int(np.ceil(float(F(F(R) + F(w))))) + 1                          # attr_ref.closest's
    m = sdf_ref.min_dist2(pos, n, reach) if len(pos) else np.full((n, n, n), np.inf, F)
    d2 = np.where(act, m, F(np.inf)).astype(F)
    return val, act, gid, v32, d2


def rank_record(pos, vel, ids, n, R, w, dx):
    """dict(origin (k, 3), values (k, 512), active (k, 512) bool, id (k, 512) uint32, velocity (k, 3, 512), dist2 (k, 512))."""
    val, act, gid, v32, d2 = _dense(pos, vel, ids, n, R, w, dx)
    bg = sdf_ref.constants(R, w, dx)[3]
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    li, lv = attr_ref.leaf_attr(gid, v32, org)
    return dict(origin=org, values=v, active=a, id=li, velocity=lv, dist2=_leaf_scalar(d2, org, F(np.inf)))


def merged(pos, vel, ids, n, R, w, dx):
    """The merge of any split of the particles: dict(origin, values, active, id, velocity) of the union."""
    r = rank_record(pos, vel, ids, n, R, w, dx)
    del r["dist2"]
    return r
