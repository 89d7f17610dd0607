"""numpy restatement of FLIPadvect (fluid.cc:972-1038) with CatmullRomFLIP (fluid.cc:210-263) and the PIC blend.

Not a conftest: tests import it.  Restated from the reference and include/fluid_hip.h, never from the kernels, in the
reference's order of operations, so that it can be held bit for bit against the oracle and the device:
  - cell_velocity: getVelocity (fluid.cc:58-70), the face average (u[c] + u[c+1]) / 2 with 0 past the last face;
  - gather: the 3 x 3 x 3 cells around round(p) in x, y, z order, each counted iff it lies within W = [2, N-3] on every
    axis; the particle is updated iff the weights sum to != 0; blend b < 1: b (v + d/w) + (1 - b) (q/w);
  - max_speed / timestep: a NaN speed never raises the maximum; dt = min(max_dt, dx / maxSpeed), max_dt when it is 0;
  - advect: the move and the stuck-particle branch with e = 0 (C round on the moved axis, C truncation toward zero on the
    two others; isSolid is false off the grid and for a non-finite coordinate).
Everything is vectorised over particles (rows of (m, 3) arrays).
"""
import numpy as np

import sources_ref as sr

CHUNK = 1 << 20   # particles per pass of the gather (bounds the temporaries at size)
PATH_G2P_TILES = 1024   # include/fluid_hip.h FLUID_PATH_G2P_TILES: the gather went through k_g2p_tiled


def cell_velocity(vel):
    """getVelocity over the whole grid: (3, n, n, n) face values -> (3, n, n, n) cell averages (0 past the last face)."""
    vel = np.asarray(vel, dtype=np.float64)
    out = np.empty_like(vel)
    for a in range(3):
        nxt = np.zeros_like(vel[a])
        sl = [slice(None)] * 3
        sl[a] = slice(0, -1)
        src = [slice(None)] * 3
        src[a] = slice(1, None)
        nxt[tuple(sl)] = vel[a][tuple(src)]
        out[a] = (vel[a] + nxt) / 2.0
    return out


def gather(n, vel, vel_before, pos, pvel, blend=1.0, wbound=None):
    """CatmullRomFLIP for every particle: the new velocities (m, 3).  wbound: the inclusive index range of W on every axis
    ((2, n - 3); other values only to show that a test discriminates)."""
    pos = np.asarray(pos, dtype=np.float64)
    pvel = np.asarray(pvel, dtype=np.float64)
    glo = -(n // 2)
    wlo, whi = (2, n - 3) if wbound is None else wbound
    cn = cell_velocity(vel)
    cb = cell_velocity(vel_before)
    dc = (cn - cb).reshape(3, -1)         # velc - velp per cell (fluid.cc:252)
    pc = cn.reshape(3, -1)                # velc (clampedCatmullRom's gather, fluid.cc:163-174)
    del cn, cb
    out = pvel.copy()
    for s in range(0, len(pos), CHUNK):
        p = pos[s:s + CHUNK]
        base = sr.c_round(p).astype(np.int64) - glo   # index of round(p) (finite positions within +-2^31)
        m = len(p)
        weight = np.zeros(m)
        d = np.zeros((3, m))
        q = np.zeros((3, m))
        sp = [[sr.spline(p[:, a] - (base[:, a] + k + glo)) for k in (-1, 0, 1)] for a in range(3)]
        inax = [[(base[:, a] + k >= wlo) & (base[:, a] + k <= whi) for k in (-1, 0, 1)] for a in range(3)]
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    inw = inax[0][i] & inax[1][j] & inax[2][k]
                    lin = ((np.where(inw, base[:, 0] + i - 1, 0) * n + np.where(inw, base[:, 1] + j - 1, 0)) * n
                           + np.where(inw, base[:, 2] + k - 1, 0))
                    cw = (sp[0][i] * sp[1][j]) * sp[2][k]
                    weight = np.where(inw, weight + cw, weight)
                    for a in range(3):
                        d[a] = np.where(inw, d[a] + dc[a][lin] * cw, d[a])
                        if blend < 1.0:
                            q[a] = np.where(inw, q[a] + pc[a][lin] * cw, q[a])
        upd = weight != 0
        v = out[s:s + CHUNK]
        w = weight[upd]
        for a in range(3):
            va = v[upd, a] + d[a][upd] / w
            if blend < 1.0:
                va = blend * va + (1.0 - blend) * (q[a][upd] / w)
            v[upd, a] = va
    return out


def speeds(pvel):
    """Vec3::length of every row: sqrt((x*x + y*y) + z*z)."""
    v = np.asarray(pvel, dtype=np.float64)
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def max_speed(pvel):
    """fluid.cc:982: maxSpeed < len, so a NaN speed never raises the maximum (0 with no particle)."""
    s = speeds(pvel)
    s = s[~np.isnan(s)]
    return float(s.max()) if len(s) else 0.0


def timestep(max_speed_, max_dt, dx):
    """fluid.cc:992-999."""
    if max_speed_ != 0:
        return max_dt if max_dt < dx / max_speed_ else dx / max_speed_
    return max_dt


def is_solid(n, solid, x, y, z):
    """isSolid at world coordinates given as float arrays of integral values: false off the grid and where one is not finite."""
    glo = -(n // 2)
    c = np.stack([x, y, z], axis=1) - glo
    ok = np.all(np.isfinite(c) & (c >= 0) & (c <= n - 1), axis=1)
    i = np.where(ok[:, None], c, 0).astype(np.int64)
    return ok & (np.asarray(solid).reshape(n, n, n)[i[:, 0], i[:, 1], i[:, 2]] != 0)


def advect(n, solid, pos, pvel, max_dt=0.1, dx=1.0, dt=None, trunc=np.trunc, rnd=sr.c_round):
    """fluid.cc:992-1036 after the gather: (positions, velocities, dt).  dt=None: from max_speed(pvel); else the given dt.
    trunc: Coord(double, double, double)'s conversion of the two untouched axes; rnd: C round on the moved axes (other
    functions, e.g. np.floor for trunc or np.rint for rnd, only to show that a test discriminates)."""
    P = np.array(pos, dtype=np.float64)
    V = np.array(pvel, dtype=np.float64)
    if dt is None:
        dt = timestep(max_speed(V), max_dt, dx)
    e = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        moved = P + dt * V
        r = rnd(moved)
        stuck = is_solid(n, solid, r[:, 0], r[:, 1], r[:, 2])
        Ps, Vs = P[stuck], V[stuck]
        vd = Vs * dt
        t = trunc(Ps)
        for a in range(3):
            c = [t[:, 0], t[:, 1], t[:, 2]]
            c[a] = rnd(Ps[:, a] + vd[:, a])
            hit = is_solid(n, solid, *c)
            Vs[hit, a] = Vs[hit, a] * (-1.0 * e)
        P[stuck] = Ps + Vs * dt
        V[stuck] = Vs
        P[~stuck] = moved[~stuck]
    return P, V, dt


def flip_advect(n, solid, vel, vel_before, pos, pvel, blend=1.0, max_dt=0.1, dx=1.0, wbound=None, trunc=np.trunc, rnd=sr.c_round):
    """The whole phase: (positions, velocities, max_speed, dt)."""
    v = gather(n, vel, vel_before, pos, pvel, blend, wbound)
    ms = max_speed(v)
    dt = timestep(ms, max_dt, dx)
    p, v, _ = advect(n, solid, pos, v, dt=dt, trunc=trunc, rnd=rnd)
    return p, v, ms, dt


# ---- scenes shared by tests/test_flip_ref.py and tests/test_gpu_g2p.py ------------------------------------------------

def default_solid(n):
    """The solid shell every scene has: the cells outside W."""
    s = np.zeros((n, n, n), dtype=np.uint8)
    s[:2] = s[-2:] = 1
    s[:, :2] = s[:, -2:] = 1
    s[:, :, :2] = s[:, :, -2:] = 1
    return s


def adversarial_fields(n, rng, outside=1e3):
    """Independent random face values everywhere for vel and velBefore: O(1) within W, `outside` times that elsewhere (the
    shell and past it), so that a cell read across the W bound shows."""
    idx = np.arange(n)
    inw1 = (idx >= 2) & (idx <= n - 3)
    inw = inw1[:, None, None] & inw1[None, :, None] & inw1[None, None, :]
    scale = np.where(inw, 1.0, outside)
    return [rng.standard_normal((3, n, n, n)) * scale for _ in range(2)]


def cells_points(cells, per_cell, rng, glo):
    """per_cell uniform points in each index cell (m, 3) of `cells` (world coordinates)."""
    c = np.repeat(np.asarray(cells, dtype=np.float64), per_cell, axis=0) + glo
    return c + rng.uniform(-0.5, 0.5, size=c.shape)


def box_cells(lo, hi):
    """The index cells of the inclusive box [lo, hi] (m, 3)."""
    g = np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij")
    return np.stack([x.ravel() for x in g], axis=1)


def aimed(n, solid, rng, per_face=40, speed=8.0, spread=2.0):
    """Particles next to every face of a solid region, moving into it: for each solid cell face that borders a fluid cell
    within W (sampled), a point within half a cell of the face on the fluid side, velocity `speed` toward the face plus a
    random tangential part.  Returns (pos, vel) in world coordinates."""
    glo = -(n // 2)
    s = np.asarray(solid).astype(bool)
    pos, vel = [], []
    idx = np.arange(n)
    inw1 = (idx >= 2) & (idx <= n - 3)
    inw = inw1[:, None, None] & inw1[None, :, None] & inw1[None, None, :]
    for a in range(3):
        for sgn in (-1, 1):
            # fluid cell c with a solid neighbour at c + sgn e_a
            nb = np.roll(s, -sgn, axis=a)
            cand = np.argwhere(inw & ~s & nb)
            if len(cand) == 0:
                continue
            pick = cand[rng.choice(len(cand), size=min(per_face, len(cand)), replace=False)]
            p = pick.astype(np.float64) + glo + rng.uniform(-0.45, 0.45, size=pick.shape)
            p[:, a] = pick[:, a] + glo + sgn * rng.uniform(0.0, 0.49, size=len(pick))
            v = rng.uniform(-spread, spread, size=pick.shape)
            v[:, a] = sgn * speed * rng.uniform(0.8, 1.0, size=len(pick))
            pos.append(p)
            vel.append(v)
    return np.concatenate(pos), np.concatenate(vel)


def obstacle_solid(n):
    """test_edge_obstacle's block on the floor plus a floating block at negative coordinates (every face reachable)."""
    s = default_solid(n)
    s[4:28, 2:9, 12:15] = 1
    s[9:13, 11:14, 5:9] = 1
    return s


def edge_particles(n, rng):
    """Half-integer ties on both sides of zero, the shell, past the grid, 1e6 (pos, vel)."""
    lo, hi = -(n // 2), -(n // 2) + n - 1
    ties = np.array([[0.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [1.5, -2.5, 3.5], [-3.5, 2.5, -1.5], [2.5, -0.5, 0.0],
                     [-4.5, -6.5, -5.5], [lo + 1.5, lo + 2.5, hi - 2.5], [hi - 1.5, -0.5, lo + 1.5]])
    shell = np.concatenate([rng.uniform(lo - 0.4, lo + 1.6, size=(20, 3)), rng.uniform(hi - 1.6, hi + 0.4, size=(20, 3)),
                            rng.uniform(lo - 0.4, hi + 0.4, size=(40, 3))])
    off = np.array([[hi + 3.0, 0.0, 0.0], [0.0, lo - 7.5, 0.0], [lo - 1.2, lo - 1.6, 2.0], [1e6, -1e6, 3.0], [1e6, 1e6, 1e6]])
    pos = np.concatenate([ties, shell, off])
    return pos, rng.standard_normal(pos.shape) * 3.0


def tie_solid(n):
    """obstacle_solid plus a block at positive coordinates (world x 6..8, y 2..4, z 4..6) whose + faces lie at even
    coordinates: there the tie beyond the face rounds away from zero into the fluid cell but to even into the block."""
    s = obstacle_solid(n)
    glo = -(n // 2)
    s[6 - glo:9 - glo, 2 - glo:5 - glo, 4 - glo:7 - glo] = 1
    return s


TIE_DT = 0.125   # a power-of-two max_dt: P + dt v is exact for the tie particles


def tie_particles(n, solid, rng, per_face=None):
    """Particles whose moved coordinate on one axis is exactly the half-integer between a fluid cell within W and its solid
    neighbour: start at the fluid cell's centre (integer coordinates), 4 cells/s toward the face on that axis, under 1 on
    the two others, so that with dt = TIE_DT (maxSpeed < 8, dx = 1) the move on that axis is exactly 0.5.  The gather must
    leave the velocities as they are (vel == velBefore, blend 1).  per_face: at most that many per axis and side (None: every
    such face).  Returns (pos, vel, axis of the tie)."""
    glo = -(n // 2)
    s = np.asarray(solid).astype(bool)
    idx = np.arange(n)
    inw1 = (idx >= 2) & (idx <= n - 3)
    inw = inw1[:, None, None] & inw1[None, :, None] & inw1[None, None, :]
    pos, vel, axis = [], [], []
    for a in range(3):
        for sgn in (-1, 1):
            cand = np.argwhere(inw & ~s & np.roll(s, -sgn, axis=a))
            if per_face is not None:
                cand = cand[rng.choice(len(cand), size=min(per_face, len(cand)), replace=False)]
            pick = cand
            v = rng.uniform(-1.0, 1.0, size=pick.shape)
            v[:, a] = 4.0 * sgn
            pos.append((pick + glo).astype(np.float64))
            vel.append(v)
            axis.append(np.full(len(pick), a))
    return np.concatenate(pos), np.concatenate(vel), np.concatenate(axis)


def floor_half_up(x):
    """floor(x + 0.5): another rounding a kernel might use (discrimination only)."""
    return np.floor(np.asarray(x, dtype=np.float64) + 0.5)


def tie_changes(n, solid, U, pos, vel, axis, got, rnd):
    """A tie scene restated with another rounding `rnd` on the moved axes: (changed particles with a negative tie, changed
    particles with a positive tie) against `got`, the C-round result (p, v, ...)."""
    t = (pos + TIE_DT * vel)[np.arange(len(pos)), axis]
    p, v, _, _ = flip_advect(n, solid, U, U, pos, vel, max_dt=TIE_DT, rnd=rnd)
    d = np.any((p != got[0]) | (v != got[1]), axis=1)
    return int((d & (t < 0)).sum()), int((d & (t > 0)).sum())
