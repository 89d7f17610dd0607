"""Reference for the liquid surface (include/fluid_hip.h, "liquid surface") — test infrastructure, numpy only.

The narrow-band level set of spheres of a fixed radius around the particles, as OpenVDB's ParticlesToLevelSet leaves it
(tools/ParticlesToLevelSet.h:591-643, rasterFixedSpheres), clipped to the grid [lo,hi]^3, in float32 / float64 exactly as
the header states them:
  sequential()  the loop of lines 591-643 restated particle by particle on a dense grid (probeValue, setValueOff(inside),
                `if (d < v) setValue`), in the order the particles are given;
  closed()      the same grid as a function of the minimum squared distance per voxel, vectorised;
  leaf_list()   the leaves that hold anything but inactive +background, ascending (x, y, z).
"""
import numpy as np

F = np.float32


def geometry(n):
    lo = -(n // 2)
    hi = lo + n - 1
    l0 = lo & ~7
    nl = ((hi & ~7) - l0) // 8 + 1
    return lo, hi, l0, nl


def constants(R, w, dx):
    """(R, w, dxf, bg, max2, min2), every operation in float32."""
    R, w, dxf = F(R), F(w), F(dx)
    mx = F(R + w)
    mn = max(F(0), F(R - w))
    return R, w, dxf, F(dxf * w), F(mx * mx), F(mn * mn)


def base_cell(p):
    """C round(): halves away from zero (p - trunc(p) is exact in double)."""
    p = np.asarray(p, dtype=np.float64)
    t = np.trunc(p)
    f = p - t
    return (t + np.where(f >= 0.5, 1.0, 0.0) - np.where(f <= -0.5, 1.0, 0.0)).astype(np.int64)


def counted(pos, n):
    """The particles whose base cell lies in the grid, and their base cells."""
    lo, hi, _, _ = geometry(n)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    c = base_cell(pos)
    keep = ((c >= lo) & (c <= hi)).all(axis=1)
    return pos[keep], c[keep]


def dist2(cx, cy, cz, P):
    """x2y2z2 of the voxel(s) (cx, cy, cz) and the particle(s) P[..., 3]: double differences and squares, float after each axis."""
    ax = np.asarray(cx, dtype=np.float64) - P[..., 0]
    ay = np.asarray(cy, dtype=np.float64) - P[..., 1]
    az = np.asarray(cz, dtype=np.float64) - P[..., 2]
    x2 = (ax * ax).astype(F)
    x2y2 = (x2.astype(np.float64) + ay * ay).astype(F)
    return (x2y2.astype(np.float64) + az * az).astype(F)


def sequential(pos, n, R, w, dx):
    """Lines 591-643, one particle after the other; voxels outside [lo,hi]^3 are not touched.  (values, active) (n, n, n)."""
    lo, hi, _, _ = geometry(n)
    R, w, dxf, bg, max2, min2 = constants(R, w, dx)
    mx = float(F(R + w))
    val = np.full((n, n, n), bg, dtype=F)
    act = np.zeros((n, n, n), dtype=bool)
    P, _ = counted(pos, n)
    for p in P:
        a = np.floor(p - mx).astype(int)
        b = np.ceil(p + mx).astype(int)
        for cx in range(max(a[0], lo), min(b[0], hi) + 1):
            x2 = F((cx - p[0]) * (cx - p[0]))
            for cy in range(max(a[1], lo), min(b[1], hi) + 1):
                x2y2 = F(np.float64(x2) + (cy - p[1]) * (cy - p[1]))
                for cz in range(max(a[2], lo), min(b[2], hi) + 1):
                    d2 = F(np.float64(x2y2) + (cz - p[2]) * (cz - p[2]))
                    i = (cx - lo, cy - lo, cz - lo)
                    v = val[i]
                    if d2 >= max2 or (not act[i] and v < 0):
                        continue
                    if d2 <= min2:
                        val[i], act[i] = -bg, False
                        continue
                    d = F(dxf * F(np.sqrt(d2) - R))
                    if d < v:
                        val[i], act[i] = d, True
    return val, act


def min_dist2(pos, n, reach):
    """m (n, n, n) float32: the minimum x2y2z2 over the counted particles whose base cell is within `reach` cells (inf: none)."""
    lo, hi, _, _ = geometry(n)
    P, c = counted(pos, n)
    m = np.full(n * n * n, np.inf, dtype=F)
    r = np.arange(-reach, reach + 1)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    step = max(1, 2_000_000 // len(off))
    for s in range(0, len(P), step):
        v = c[s:s + step, None, :] + off[None, :, :]                      # (p, o, 3) voxel coordinates
        ok = ((v >= lo) & (v <= hi)).all(axis=2)
        d = dist2(v[..., 0], v[..., 1], v[..., 2], P[s:s + step, None, :])
        idx = ((v[..., 0] - lo) * n + (v[..., 1] - lo)) * n + (v[..., 2] - lo)
        np.minimum.at(m, idx[ok], d[ok])
    return m.reshape(n, n, n)


def closed(pos, n, R, w, dx):
    """The grid as a function of the particle set: (values, active) (n, n, n)."""
    R, w, dxf, bg, max2, min2 = constants(R, w, dx)
    # a particle at less than mx from a voxel has its base cell at most ceil(mx) cells away; further ones cannot change the voxel
    m = min_dist2(pos, n, int(np.ceil(float(F(R + w)))) + 1)
    with np.errstate(invalid="ignore"):
        d = (dxf * (np.sqrt(m) - R).astype(F)).astype(F)
    band = (m < max2) & ~(m <= min2)
    act = band & (d < bg)
    val = np.full(m.shape, bg, dtype=F)
    val[m <= min2] = -bg
    val[act] = d[act]
    return val, act


def leaf_list(val, act, bg):
    """(origin (k, 3) int32, values (k, 512) float32, active (k, 512) bool): the leaves with an in-grid voxel that is anything but
    inactive +bg, ascending (x, y, z); voxels outside the grid are inactive +bg."""
    n = val.shape[0]
    lo, hi, l0, nl = geometry(n)
    pad = nl * 8
    o = lo - l0
    V = np.full((pad,) * 3, F(bg), dtype=F)
    A = np.zeros((pad,) * 3, dtype=bool)
    V[o:o + n, o:o + n, o:o + n] = val
    A[o:o + n, o:o + n, o:o + n] = act
    V = V.reshape(nl, 8, nl, 8, nl, 8).transpose(0, 2, 4, 1, 3, 5).reshape(nl ** 3, 512)
    A = A.reshape(nl, 8, nl, 8, nl, 8).transpose(0, 2, 4, 1, 3, 5).reshape(nl ** 3, 512)
    listed = (A | (V.view(np.uint32) != np.array(bg, dtype=F).view(np.uint32))).any(axis=1)
    k = np.flatnonzero(listed)
    org = np.stack([k // (nl * nl), (k // nl) % nl, k % nl], axis=1) * 8 + l0
    return org.astype(np.int32), np.ascontiguousarray(V[k]), np.ascontiguousarray(A[k])
