"""numpy restatements for the particle sources and sinks (include/fluid_hip.h, "particle sources and sinks").

Not a conftest: tests import it.  Everything here is restated from the header and the reference, never from the kernels:
  - sm64 / source_points: where a source puts its points (SplitMix64 of seed, step, cell, k) and which of them it keeps;
  - clamped_catmull_rom: the reference's clampedCatmullRom (fluid.cc:125-207) over getVelocity's cell averages
    (fluid.cc:58-70), i.e. what PointList::interpFromGrid (fluid.cc:883-894) gives a new point.
"""
import numpy as np

MASK = (1 << 64) - 1


def sm64_int(x):
    """SplitMix64 on one Python int (the hand-checkable form)."""
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sm64(x):
    """SplitMix64 over a uint64 array (wrapping arithmetic)."""
    z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def cell_points(n, seed, t, linear, coords, k):
    """Point k of the cells `linear` (int64 array) with coordinates coords (m, 3): positions (m, 3) and the keep mask."""
    h0 = sm64_int(sm64_int(seed & MASK) ^ (t & MASK))
    with np.errstate(over="ignore"):
        h = sm64(np.uint64(h0) ^ np.asarray(linear, dtype=np.uint64))
        key = h ^ np.uint64(k)
        p = np.empty((len(linear), 3))
        for a in range(3):
            u = (sm64(key + np.uint64(a)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
            p[:, a] = coords[:, a].astype(np.float64) + (u - 0.5)
    keep = np.all(c_round(p) == coords, axis=1)
    return p, keep


def c_round(x):
    """C round(): half away from zero (numpy's round is half to even); x - trunc(x) is exact."""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= 0.5, t + np.copysign(1.0, x), t)


def default_solid(n):
    """The solid array of a handle that fluid_set_solid was never called on: the two outer layers."""
    s = np.zeros((n, n, n), dtype=np.uint8)
    s[:2] = s[-2:] = 1
    s[:, :2] = s[:, -2:] = 1
    s[:, :, :2] = s[:, :, -2:] = 1
    return s


def base_cells(n, pos):
    """Index of the base cell round(p) of every row of pos."""
    return c_round(pos).astype(np.int64) + n // 2


def eligible_cells(n, lo, hi, solid):
    """The eligible cells of the inclusive index box [lo, hi] in ascending linear order: (linear, index (m, 3))."""
    ix, iy, iz = np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij")
    idx = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.int64)
    inw = np.all((idx >= 2) & (idx <= n - 3), axis=1)
    idx = idx[inw]
    lin = (idx[:, 0] * n + idx[:, 1]) * n + idx[:, 2]
    ok = np.asarray(solid).reshape(-1)[lin] == 0
    return lin[ok], idx[ok]


def base_cell_counts(n, lo, hi, pos):
    """Particles per base cell round(p) over the box (shape of the box), like the FILL histogram."""
    glo = -(n // 2)
    c = c_round(np.asarray(pos)) - glo
    shape = tuple(hi[a] - lo[a] + 1 for a in range(3))
    inside = np.all((c >= lo) & (c <= hi), axis=1)
    loc = (c[inside] - lo).astype(np.int64)
    h = np.zeros(shape, dtype=np.int64)
    np.add.at(h, (loc[:, 0], loc[:, 1], loc[:, 2]), 1)
    return h


def source_points(n, seed, t, lo, hi, per_cell, solid, hist=None):
    """The points a source emits at step t, in pid order (ascending linear cell, then k).  hist (box-shaped counts): FILL."""
    glo = -(n // 2)
    lin, idx = eligible_cells(n, lo, hi, solid)
    if hist is None:
        tries = np.full(len(lin), per_cell, dtype=np.int64)
    else:
        loc = idx - np.asarray(lo)
        tries = np.maximum(0, per_cell - hist[loc[:, 0], loc[:, 1], loc[:, 2]])
    coords = idx + glo
    pts = np.empty((len(lin), per_cell, 3))
    kept = np.zeros((len(lin), per_cell), dtype=bool)
    for k in range(per_cell):
        p, keep = cell_points(n, seed, t, lin, coords, k)
        pts[:, k] = p
        kept[:, k] = keep & (k < tries)
    return pts[kept]


def spline(x):
    """fluid.cc:22-37, the same operations in the same order."""
    x = np.abs(x)
    a = 1.5 * ((((4.0 * x) * x) * x - (4.0 * x) * x) + 2.0 / 3.0)
    b = 1.5 * (((((-8.0 * ((x * x) * x)) / 6.0) + (4.0 * x) * x) - 4.0 * x) + 4.0 / 3.0)
    return np.where(x < 0.5, a, np.where(x < 1.0, b, 0.0))


def clamped_catmull_rom(n, vel, pos):
    """clampedCatmullRom(p, vels, bound, ..) for every row of pos over FLUID_FIELD_VEL (3, n, n, n): cells outside W skipped,
    (0, 0, 0) where the weights sum to 0.  The cells are visited x, then y, then z, like the reference's loops."""
    pos = np.asarray(pos, dtype=np.float64)
    glo = -(n // 2)
    wlo, whi = glo + 2, glo + n - 1 - 2
    u, v, w = vel[0], vel[1], vel[2]
    f = c_round(pos).astype(np.int64)
    m = len(pos)
    weight = np.zeros(m); su = np.zeros(m); sv = np.zeros(m); sw = np.zeros(m)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                c = f + np.array([dx, dy, dz])
                inw = np.all((c >= wlo) & (c <= whi), axis=1)
                i = np.where(inw[:, None], c - glo, 2)   # a readable index where the cell is skipped
                x, y, z = i[:, 0], i[:, 1], i[:, 2]
                cu = (u[x, y, z] + u[x + 1, y, z]) / 2.0
                cv = (v[x, y, z] + v[x, y + 1, z]) / 2.0
                cw_ = (w[x, y, z] + w[x, y, z + 1]) / 2.0
                cw = (spline(pos[:, 0] - c[:, 0]) * spline(pos[:, 1] - c[:, 1])) * spline(pos[:, 2] - c[:, 2])
                weight = np.where(inw, weight + cw, weight)
                su = np.where(inw, su + cu * cw, su)
                sv = np.where(inw, sv + cv * cw, sv)
                sw = np.where(inw, sw + cw_ * cw, sw)
    out = np.zeros((m, 3))
    nz = weight != 0
    out[nz, 0] = su[nz] / weight[nz]
    out[nz, 1] = sv[nz] / weight[nz]
    out[nz, 2] = sw[nz] / weight[nz]
    return out
