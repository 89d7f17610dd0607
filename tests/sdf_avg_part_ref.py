"""Reference for the rank records of the averaged-position surface and their merge (include/fluid_hip.h, "liquid surface, averaged
positions (decomposed runs)") — test infrastructure, numpy on top of sdf_avg_ref.sums / finish and sdf_ref's leaf layout.

record(): the canonical record of a particle set: the leaves with an in-grid voxel of m < reach2 = max(max2, h2), and per voxel
dist2 = m inside (min2, reach2), +0 at or below min2, +inf elsewhere, with the four sums kept only in the first case.
merge(): minimum of dist2, wrapping sums of the sums, sdf_avg_ref.finish, and the list of the leaves with anything but inactive +bg.
"""
import numpy as np

import sdf_avg_ref
import sdf_ref

F = np.float32
LEAF_BYTES = 2048 + 4 * 4096 + 12                          # FLUID_SDF_AVG_PART_LEAF_BYTES


def to_leaves(a, n, fill):
    """(nl^3, 512) of an (n, n, n) array, the voxels outside the grid holding `fill`; leaf index (x * nl + y) * nl + z."""
    lo, _, l0, nl = sdf_ref.geometry(n)
    o = lo - l0
    V = np.full((nl * 8,) * 3, fill, dtype=a.dtype)
    V[o:o + n, o:o + n, o:o + n] = a
    return V.reshape(nl, 8, nl, 8, nl, 8).transpose(0, 2, 4, 1, 3, 5).reshape(nl ** 3, 512)


def origins(k, n):
    _, _, l0, nl = sdf_ref.geometry(n)
    return (np.stack([k // (nl * nl), (k // nl) % nl, k % nl], axis=1) * 8 + l0).astype(np.int32)


def reach2(R, w, dx, h):
    _, _, _, _, max2, _ = sdf_ref.constants(R, w, dx)
    return max(max2, sdf_avg_ref.constants(h)[0])


def record(pos, n, R, w, dx, h):
    """(origin (k, 3) int32 ascending, dist2 (k, 512) float32, sums (k, 4, 512) uint64) of the particles `pos`."""
    _, _, _, _, _, min2 = sdf_ref.constants(R, w, dx)
    r2 = reach2(R, w, dx, h)
    m, *S = sdf_avg_ref.sums(pos, n, h)
    keep = (m > min2) & (m < r2)
    d2 = np.where(keep, m, np.where(m <= min2, F(0.0), F(np.inf))).astype(F)
    D = to_leaves(d2, n, F(np.inf))
    SS = np.stack([to_leaves(np.where(keep, s, 0).astype(np.int64).view(np.uint64), n, np.uint64(0)) for s in S], axis=1)
    k = np.flatnonzero((to_leaves(m, n, F(np.inf)) < r2).any(axis=1))
    return origins(k, n), np.ascontiguousarray(D[k]), np.ascontiguousarray(SS[k])


def merge(records, n, R, w, dx):
    """(origin (k, 3) int32, values (k, 512) float32, active (k, 512) bool) of the union, from records as record() gives them."""
    _, _, l0, nl = sdf_ref.geometry(n)
    bg = sdf_ref.constants(R, w, dx)[3]
    M = np.full((nl ** 3, 512), np.inf, dtype=F)
    S = np.zeros((nl ** 3, 4, 512), dtype=np.uint64)
    for org, d2, sums in records:
        if not len(org):
            continue
        c = (np.asarray(org, dtype=np.int64) - l0) // 8
        j = (c[:, 0] * nl + c[:, 1]) * nl + c[:, 2]
        M[j] = np.minimum(M[j], d2)
        S[j] += sums                                           # uint64: wraps
    Si = S.view(np.int64)
    val, act = sdf_avg_ref.finish(M, Si[:, 0], Si[:, 1], Si[:, 2], Si[:, 3], R, w, dx)
    k = np.flatnonzero((act | (val.view(np.uint32) != np.array(bg, dtype=F).view(np.uint32))).any(axis=1))
    return origins(k, n), np.ascontiguousarray(val[k]), np.ascontiguousarray(act[k])


def two_particles():
    """n, (R, w, dx, h), A, B of the list rule's scene: base cells -1 and 2 along x, either side of the uniform cut of 2x1x1 at
    n = 16; B weighs on voxels inside A's band where B's own spheres' list has no leaf."""
    return 16, (1.0, 1.0, 1.0, 4.0), np.array([[-0.6, 0.0, 0.0]]), np.array([[1.5, 0.0, 0.0]])
