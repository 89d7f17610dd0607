"""Reference for the velocity trails (include/fluid_hip.h, "liquid surface, velocity trails") — test infrastructure, numpy only.
It knows no leaves and no cells: instances() expands the particles element-wise in the float32 / float64 types of the definition,
union() evaluates every voxel against every counted item by brute force; constants, base cells, x2y2z2 and the leaf list are
sdf_ref's.

The one shortcut of union(): a voxel row (cx, cy, all cz) looks only at the items with |Px - cx| < 5 and |Py - cy| < 5.  Any other
has x2 >= 25 as computed (the x or the y term alone is, and every later rounding is monotone), which is above every item's
max2 <= 16: it says nothing.  A bound on a distance, not a walk over cells.
"""
import functools

import numpy as np

import sdf_ref

F = np.float32
FLT_MAX = np.finfo(F).max


def instances(pos, vel, R, trails):
    """(positions float64 (k, 3), radii float32 (k,), particle index (k,)) in particle order, a particle's instances in the order
    they are made.  trails = (shutter, delta, radius_min, max_instances)."""
    shutter, delta, rmin, maxi = trails
    P0 = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    R, Rm = F(R), F(rmin)
    c, dR = F(F(0.5) * F(delta)), F(R - Rm)
    n = len(P0)
    with np.errstate(all="ignore"):
        vf = (np.float64(shutter) * v).astype(F)
        s2 = (vf[:, 0] * vf[:, 0] + vf[:, 1] * vf[:, 1]) + vf[:, 2] * vf[:, 2]
        speed = np.sqrt(s2)
        alive = (speed > F(0)) & (speed <= FLT_MAX)
        inv = np.where(alive, F(1) / np.where(alive, speed, F(1)), F(0)).astype(F)
        nrm = -(vf * inv[:, None])
        t = np.zeros(n, dtype=F)
        r = np.full(n, R, dtype=F)
        who, P, rad, order = [np.arange(n)], [P0], [r.copy()], [np.zeros(n, dtype=np.int64)]
        for k in range(1, int(maxi)):
            t = np.where(alive, t + c * r, t).astype(F)
            alive = alive & (t <= speed)
            if not alive.any():
                break
            r = np.where(alive, R - (dR * t) * inv, r).astype(F)
            i = np.flatnonzero(alive)
            step = (t[i, None] * nrm[i]).astype(F)
            who.append(i), P.append(P0[i] + step.astype(np.float64)), rad.append(r[i]), order.append(np.full(len(i), k, dtype=np.int64))
    who, P, rad, order = np.concatenate(who), np.vstack(P), np.concatenate(rad), np.concatenate(order)
    o = np.lexsort((order, who))
    return P[o], rad[o], who[o]


def union(items, radii, n, R, w, dx):
    """(values, active) (n, n, n) of the items (positions (k, 3), radii (k,) float32, each <= R) by the voxel rule."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    _, w, dxf, bg, _, _ = sdf_ref.constants(R, w, dx)
    P = np.asarray(items, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(radii, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore"):
        c = sdf_ref.base_cell(np.where(np.isfinite(P), P, 1e300))
    keep = ((c >= lo) & (c <= hi)).all(axis=1) & np.isfinite(P).all(axis=1)
    P, r = P[keep], r[keep]
    mx = (r + w).astype(F)
    max2 = (mx * mx).astype(F)
    mn = np.maximum(F(0), (r - w).astype(F))
    min2 = (mn * mn).astype(F)
    inside = np.zeros((n, n, n), dtype=bool)
    best = np.full((n, n, n), np.inf, dtype=F)
    cz = np.arange(lo, hi + 1)
    for ix in range(n):
        cx = lo + ix
        nx = np.flatnonzero(np.abs(P[:, 0] - cx) < 5.0)
        for iy in range(n):
            cy = lo + iy
            q = nx[np.abs(P[nx, 1] - cy) < 5.0]
            if not len(q):
                continue
            x2 = sdf_ref.dist2(cx, cy, cz[:, None], P[None, q, :])                  # (n, items)
            says = ~(x2 >= max2[q])
            ins = says & (x2 <= min2[q])
            cand = says & ~ins
            with np.errstate(invalid="ignore"):
                d = (dxf * (np.sqrt(x2) - r[q]).astype(F)).astype(F)
            inside[ix, iy] = ins.any(axis=1)
            best[ix, iy] = np.where(cand, d, F(np.inf)).min(axis=1)
    act = ~inside & (best < bg)
    val = np.full((n, n, n), bg, dtype=F)
    val[inside] = -bg
    val[act] = best[act]
    return val, act


def trails_surface(pos, vel, n, R, w, dx, trails):
    """The grid of the particles' trails: (values, active)."""
    P, r, _ = instances(pos, vel, R, trails)
    return union(P, r, n, R, w, dx)


def merge(a, b, bg):
    """The rule of fluid_sdf_grids_merge on two dense grids (values, active): -bg wins, then the smallest active value, else +bg."""
    (va, aa), (vb, ab) = a, b
    neg = (~aa & (va < 0)) | (~ab & (vb < 0))
    act = ~neg & (aa | ab)
    val = np.full(va.shape, F(bg), dtype=F)
    val[neg] = -F(bg)
    m = np.minimum(np.where(aa, va, F(np.inf)), np.where(ab, vb, F(np.inf)))
    val[act] = m[act]
    return val, act


SETS = [(1.0, 3.0, 1.0), (1.5, 2.5, 1.0), (3.0, 1.0, 1.0), (1.0, 2.0, 0.5)]      # (R, w, dx)


def trails_of(R):
    """The setting the tests use with radius R: shutter 1, delta 1, the trail ends at R / 2, at most 8 instances."""
    return (1.0, 1.0, float(R) / 2, 8)


@functools.lru_cache(maxsize=None)
def block_scene(n=24, seed=24):
    """sdf_avg_ref.block_and_scattered(n) with random velocities of 0 to 6 voxels per shutter: (pos, vel), read-only."""
    import sdf_avg_ref
    pos = sdf_avg_ref.block_and_scattered(n, seed)
    rng = np.random.default_rng(seed + 1)
    d = rng.normal(size=pos.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    vel = d * rng.uniform(0.0, 6.0, (len(pos), 1))
    pos.setflags(write=False), vel.setflags(write=False)
    return pos, vel


@functools.lru_cache(maxsize=None)
def block_reference(R, w, dx, n=24):
    """(values, active, instance count) of block_scene(n) under trails_of(R): computed once per parameter set and shared."""
    pos, vel = block_scene(n)
    P, r, _ = instances(pos, vel, R, trails_of(R))
    val, act = union(P, r, n, R, w, dx)
    val.setflags(write=False), act.setflags(write=False)
    return val, act, len(P)
