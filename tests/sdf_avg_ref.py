"""Reference for the averaged-position surface (include/fluid_hip.h, "liquid surface, averaged positions") — test infrastructure,
numpy only.  It knows no leaves and no rings: every voxel row (cx, cy, all cz) meets all counted particles, in the float32,
float64 and int64 types of the definition; constants, the counted particles, x2y2z2 and the leaf list are sdf_ref's.

The one shortcut: a row looks only at the particles with |Px - cx| < 5 and |Py - cy| < 5.  Any other has x2 >= 25 as computed
(the x or the y term alone is, and every later rounding is monotone), which is above h2 <= 16 (no weight) and above max2 <= 16 (a
minimum that large is +bg whatever it is): a bound on a distance, not a walk over cells.
"""
import numpy as np

import sdf_ref

F = np.float32
W_ONE = F(16777216.0)
O_ONE = 262144.0


def block_and_scattered(n=24, seed=24):
    """The scene of test_gpu_sdf.py::test_filled_block_and_scattered: a filled block beside scattered particles, some outside."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    rng = np.random.default_rng(seed)
    c = np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    block = (np.repeat(c, 8, axis=0) + rng.uniform(-0.5, 0.5, (8 * len(c), 3)))
    return np.vstack([block, rng.uniform(lo - 1.0, hi + 1.0, (200, 3))])


def constants(influence):
    """(h2, ih2), float32."""
    hf = F(influence)
    h2 = F(hf * hf)
    return h2, F(F(1.0) / h2)


def weight(x2, h2, ih2):
    """W (int64) of the squared distances x2 (float32): 0 unless x2 < h2."""
    t = (F(1.0) - (x2 * ih2).astype(F)).astype(F)
    wt = ((t * t).astype(F) * t).astype(F)
    W = np.rint((wt * W_ONE).astype(F)).astype(np.int64)          # np.rint: half to even
    return np.where(x2 < h2, W, 0)


def offset(P, c):
    """O (int64) of particle coordinates P (float64) and voxel coordinates c (integers)."""
    return np.rint((P - np.asarray(c, dtype=np.float64)) * O_ONE).astype(np.int64)


def sums(pos, n, influence, cols=None):
    """(m float32, SW, SX, SY, SZ int64), each (n, n, n): the minimum of x2y2z2 (inf: no particle in reach) and the four sums,
    which wrap like the library's (numpy's int64 arithmetic does).  cols: the voxel rows (cx, cy) to compute (the others keep
    m = inf and sums of 0), None: all."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    h2, ih2 = constants(influence)
    P, _ = sdf_ref.counted(pos, n)
    m = np.full((n, n, n), np.inf, dtype=F)
    S = np.zeros((4, n, n, n), dtype=np.int64)
    cz = np.arange(lo, hi + 1)
    for ix in range(n):
        cx = lo + ix
        nearx = np.abs(P[:, 0] - cx) < 5.0
        Px = P[nearx]
        for iy in range(n):
            cy = lo + iy
            if cols is not None and (cx, cy) not in cols:
                continue
            Q = Px[np.abs(Px[:, 1] - cy) < 5.0]
            if not len(Q):
                continue
            x2 = sdf_ref.dist2(cx, cy, cz[:, None], Q[None, :, :])                 # (n, particles)
            m[ix, iy] = x2.min(axis=1)
            iz, ip = np.nonzero(x2 < h2)
            W = weight(x2[iz, ip], h2, ih2)
            with np.errstate(over="ignore"):
                np.add.at(S[0, ix, iy], iz, W)
                np.add.at(S[1, ix, iy], iz, W * offset(Q[ip, 0], cx))
                np.add.at(S[2, ix, iy], iz, W * offset(Q[ip, 1], cy))
                np.add.at(S[3, ix, iy], iz, W * offset(Q[ip, 2], cz[iz]))
    return m, S[0], S[1], S[2], S[3]


def finish(m, SW, SX, SY, SZ, R, w, dx):
    """(values, active) from the minimum and the sums."""
    R, w, dxf, bg, max2, min2 = sdf_ref.constants(R, w, dx)
    with np.errstate(invalid="ignore", divide="ignore"):
        ds = (dxf * (np.sqrt(m) - R).astype(F)).astype(F)
        den = SW.astype(np.float64) * O_ONE
        ax, ay, az = SX.astype(np.float64) / den, SY.astype(np.float64) / den, SZ.astype(np.float64) / den
        a2 = (ax * ax).astype(F)
        a2 = (a2.astype(np.float64) + ay * ay).astype(F)
        a2 = (a2.astype(np.float64) + az * az).astype(F)
        da = (dxf * (np.sqrt(a2) - R).astype(F)).astype(F)
        d = np.where(SW > 0, np.maximum(da, ds), ds).astype(F)
    band = (m < max2) & ~(m <= min2)
    act = band & (d < bg)
    val = np.full(m.shape, bg, dtype=F)
    val[m <= min2] = -bg
    val[act] = d[act]
    return val, act


def averaged(pos, n, R, w, dx, influence, cols=None):
    """The grid as a function of the particle set: (values, active) (n, n, n); cols as in sums()."""
    return finish(*sums(pos, n, influence, cols), R, w, dx)
