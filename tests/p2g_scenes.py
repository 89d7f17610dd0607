"""Particle sets for the particle -> grid tests (numpy only; not a conftest: test_p2g_ref.py and test_gpu_p2g.py import it).

Every builder returns (n, pos, vel, solid) with solid None or an (n, n, n) uint8 mask that already holds the shell outside W.
"""
import numpy as np

from sources_ref import c_round, spline


def bounds(n):
    lo = -(n // 2)
    return lo, lo + n - 1


def shell(n):
    s = np.ones((n, n, n), dtype=np.uint8)
    s[2:n - 2, 2:n - 2, 2:n - 2] = 0
    return s


def fill_cells(rng, lo3, hi3, per_cell):
    """Exactly per_cell(ix) particles with base cell = every cell of the inclusive coordinate box: per_cell an int or a
    (lo, hi) range drawn per cell."""
    ax = [np.arange(lo3[a], hi3[a] + 1) for a in range(3)]
    c = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    cnt = np.full(len(c), per_cell) if np.isscalar(per_cell) else rng.integers(per_cell[0], per_cell[1] + 1, size=len(c))
    c = np.repeat(c, cnt, axis=0)
    return c + rng.uniform(-0.49, 0.49, size=c.shape)


def water(n, ppc, seed=0, unit_velocity=False, full_z=False):
    """A block of evenly filled water, shuffled.  full_z: the block spans all of W along z (every z piece of a launch)."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(n)
    m = max(4, round(n * 41 / 121))
    c0 = -(m // 2)
    lo3, hi3 = [c0] * 3, [c0 + m - 1] * 3
    if full_z:
        lo3[2], hi3[2] = lo + 2, hi - 2
    pos = fill_cells(rng, lo3, hi3, ppc)
    pos = pos[rng.permutation(len(pos))]
    vel = np.ones_like(pos) if unit_velocity else rng.standard_normal(pos.shape)
    return n, pos, vel, None


def piles(seed, n=24, sizes=(60, 200, 500, 2000, 12000), background=None):
    """Random piles of 60 .. 12000 particles per cell on a thin background (given, or water(n, 2)), some in the first / last
    cell inside the walls."""
    rng = np.random.default_rng(100 + seed)
    lo, hi = bounds(n)
    parts = [water(n, 2, seed=seed)[1] if background is None else np.asarray(background)]
    for k in sizes[: 3 + seed % 3]:
        for _ in range(2):
            c = rng.integers(lo + 3, hi - 2, size=3).astype(np.float64)
            if rng.random() < 0.5:
                c[rng.integers(0, 3)] = (lo + 3) if rng.random() < 0.5 else (hi - 3)
            parts.append(c + rng.uniform(-0.49, 0.49, size=(k, 3)))
    pos = np.concatenate(parts)
    pos = pos[rng.permutation(len(pos))]
    return n, pos, rng.standard_normal(pos.shape), None


THRESHOLD_COUNTS = (17, 18, 19, 63, 64, 65, 511, 512, 513, 1024, 1025)


def thresholds(n=32, background=None):
    """Cells of exactly 17 / 18 / 19, 63 / 64 / 65, 511 / 512 / 513, 1024 / 1025 particles: alone, side by side along z, in
    wall corners, over a thin background (given, or water(n, 1))."""
    rng = np.random.default_rng(77)
    lo, hi = bounds(n)
    parts = [water(n, 1, seed=5)[1] if background is None else np.asarray(background)]
    cells = []
    for k, cnt in enumerate(THRESHOLD_COUNTS):
        cells.append(((lo + 5, lo + 6, lo + 4 + 2 * k), cnt))
    for k, cnt in enumerate(THRESHOLD_COUNTS):
        cells.append(((lo + 9, lo + 9, lo + 4 + k), cnt))
    cells += [((lo + 3, lo + 3, lo + 3), 600), ((hi - 3, hi - 3, hi - 3), 18), ((lo + 3, hi - 3, lo + 12), 513), ((hi - 3, lo + 3, hi - 3), 64)]
    for c, cnt in cells:
        parts.append(np.asarray(c, dtype=np.float64) + rng.uniform(-0.49, 0.49, size=(cnt, 3)))
    pos = np.concatenate(parts)
    pos = pos[rng.permutation(len(pos))]
    return n, pos, rng.standard_normal(pos.shape), None


def edges(n=24, seed=3, pile=300):
    """Piles and single particles in the first and the last cell inside W on every axis, in the shell outside W, off the grid
    on every side, and a solid slab cutting one pile's support."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(n)
    mid = 0.0
    parts = []
    for a in range(3):
        for end, out in ((lo + 2, -1), (hi - 2, +1)):
            c = np.array([mid, mid, mid]); c[a] = end
            parts.append(c + rng.uniform(-0.49, 0.49, size=(pile, 3)))       # a pile in the first / last cell of W
            c2 = c.copy(); c2[(a + 1) % 3] = mid + 4
            parts.append(c2[None] + rng.uniform(-0.49, 0.49, size=(1, 3)))   # one particle there
            s = c.copy(); s[a] = end + out; s[(a + 2) % 3] = mid - 4
            parts.append(s + rng.uniform(-0.49, 0.49, size=(40, 3)))         # in the shell: only its inner neighbours receive
            s2 = s.copy(); s2[a] = end + 2 * out
            parts.append(s2 + rng.uniform(-0.49, 0.49, size=(40, 3)))        # the outermost layer: nothing inside W in reach
            o = c.copy(); o[a] = end + 3 * out + out * 0.25
            parts.append(o + rng.uniform(-0.2, 0.2, size=(10, 3)))           # off the grid
            far = c.copy(); far[a] = out * 1.0e6
            parts.append(far[None].copy())
    corner = np.array([lo + 2.0, hi - 2.0, lo + 2.0])
    parts.append(corner + rng.uniform(-0.49, 0.49, size=(pile, 3)))
    ob = np.array([5.0, -5.0, 5.0])                                          # a pile whose support a solid slab cuts
    parts.append(ob + rng.uniform(-0.49, 0.49, size=(pile, 3)))
    pos = np.concatenate(parts)
    pos = pos[rng.permutation(len(pos))]
    solid = shell(n)
    i = (ob - lo).astype(int)
    solid[i[0] + 1, i[1] - 1:i[1] + 2, i[2] - 1:i[2] + 2] = 1                # the x + 1 face of the pile's support
    solid[i[0], i[1], i[2] + 1] = 1                                          # and one cell next to it
    return n, pos, rng.standard_normal(pos.shape), solid


def dense_rows(n=32, ppc=(16, 17), seed=9, unit_velocity=False):
    """Every cell of a (n - 6)^3 block holds ppc[0] .. ppc[1] particles: rows (fixed x, y) of more than 384 particles at
    n = 32; 16-17 is just under the crowded-cell threshold (no cell crowded), 18-19 just over (every cell crowded)."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(n)
    pos = fill_cells(rng, [lo + 3] * 3, [hi - 3] * 3, ppc)
    pos = pos[rng.permutation(len(pos))]
    vel = np.ones_like(pos) if unit_velocity else rng.standard_normal(pos.shape)
    return n, pos, vel, None


def on_centres(n=24, seed=4, most=3000):
    """Every particle exactly on a cell centre, integer velocities in [-8, 8], 1 .. `most` per cell: cw is exactly 1 or 0,
    every sum is exact in any order."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(n)
    ax = np.arange(lo + 3, hi - 2, 2)
    c = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    cnt = rng.integers(1, 40, size=len(c))
    cnt[rng.choice(len(c), 12, replace=False)] = [most, most - 1, 1025, 1024, 513, 512, 65, 64, 19, 18, 17, 1]
    # neighbours too: a block of adjacent centres, so that the zero-weight neighbours are other particles' cells
    blk = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64) + np.array([lo + 4.0, 0, 0])
    c = np.concatenate([c, blk])
    cnt = np.concatenate([cnt, rng.integers(1, 30, size=len(blk))])
    c, first = np.unique(c, axis=0, return_index=True)
    cnt = cnt[first]
    pos = np.repeat(c, cnt, axis=0)
    o = rng.permutation(len(pos))
    pos = pos[o]
    vel = rng.integers(-8, 9, size=pos.shape).astype(np.float64)
    return n, pos, vel, None


def ties(n=16):
    """Particles exactly on x.5 on both sides of zero (C round goes away from zero) next to ordinary ones."""
    rng = np.random.default_rng(12)
    h = np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5])
    g = np.stack(np.meshgrid(h, h, h, indexing="ij"), axis=-1).reshape(-1, 3)
    mix = g.copy()
    mix[:, 1] += rng.uniform(-0.3, 0.3, size=len(g))      # a tie on some axes only
    pos = np.concatenate([g, mix, rng.uniform(-3, 3, size=(200, 3))])
    return n, pos, rng.standard_normal(pos.shape), None


# ---- grazing addends: spline() below zero ---------------------------------------------------------------------------------
NOISE = 1.5 * 2.0 ** -52   # the spline's rounding noise next to |x| = 1 comes in multiples of this (3.33e-16)


def grazing_x(tx, side, want):
    """A coordinate x with base cell tx + side (side = +-1) whose spline value toward cell tx, spline(x - tx) as the step
    evaluates it, is exactly `want` (-NOISE or +NOISE): found by a fixed scan of 1 - 6.5e-6 < |x - tx| < 1."""
    x = tx + side * (1.0 - np.linspace(1e-9, 6.5e-6, 400001))
    hit = np.nonzero(spline(x - tx) == want)[0]
    return x[hit[len(hit) // 2]]


GRAZING_KINDS = ("neg_only", "pos_neg", "neg_pos", "cancel")


def grazing_targets(n=24):
    lo, hi = bounds(n)
    return [np.array([0.0, 0.0, 0.0]), np.array([lo + 2.0, 4.0, -4.0]), np.array([5.0, hi - 2.0, 6.0])]


def grazing(kind, n=24):
    """Cells that receive spline noise.  Each target cell T (grazing_targets) gets its addends from particles one cell away
    along x at a distance from the scan above, exactly on T's z (sz = 1) and either on T's y (sy = 1) or 0.4 off it
    (sy = spline(0.4) = 0.42: a smaller addend; its y neighbour at 0.6 receives one as well).  kinds:
      'neg_only'   one negative addend                        Wp < 0, Wc = 0
      'pos_neg'    a small positive and a larger negative     Wp < 0, Wc > 0
      'neg_pos'    a small negative and a larger positive     Wp > 0, Wc > 0, Wc != Wp
      'cancel'     a negative and the equal positive          Wp = 0, Wc > 0
      'water'      ordinary water plus a negative addend      Wp, Wc > 0 and equal at float precision
    Velocities are (1, 1, 1) so that the numerators are the weights."""
    lo, hi = bounds(n)
    rng = np.random.default_rng(31)
    g = {"neg": -NOISE, "pos": NOISE}
    parts = []
    for t in grazing_targets(n):
        side = 1.0 if t[0] == lo + 2 else -1.0            # the first cell of W has no inner neighbour on the left
        at = lambda want, sgn, dy=0.0: np.array([grazing_x(t[0], sgn, want), t[1] + dy, t[2]])
        if kind == "neg_only":
            parts += [at(g["neg"], side)]
        elif kind == "pos_neg":
            parts += [at(g["neg"], side), at(g["pos"], 1.0, 0.4)]
        elif kind == "neg_pos":
            parts += [at(g["neg"], side, 0.4), at(g["pos"], 1.0)]
        elif kind == "cancel":
            parts += [at(g["neg"], side), at(g["pos"], 1.0)]
        elif kind == "water":
            parts += [at(g["neg"], 1.0)]
            parts += list(t + rng.uniform(-0.49, 0.49, size=(8, 3)))
        else:
            raise ValueError(kind)
    pos = np.array(parts)
    if kind == "water":
        pos = np.concatenate([pos, water(n, 4, seed=8)[1] + np.array([0.0, -6.0, 0.0])])
    return n, pos, np.ones_like(pos), None


def tall_water(n, seed=None, unit_velocity=False):
    """Water over the whole z extent of W, 1 .. 24 particles per cell (cells on both sides of the crowded-cell threshold),
    16 x 16 columns."""
    rng = np.random.default_rng(n if seed is None else seed)
    lo, hi = bounds(n)
    pos = fill_cells(rng, [-8, -8, lo + 2], [7, 7, hi - 2], (1, 24))
    pos = pos[rng.permutation(len(pos))]
    vel = np.ones_like(pos) if unit_velocity else rng.standard_normal(pos.shape)
    return n, pos, vel, None


def block(n, lo3, hi3, ppc, seed):
    """A box of cells with ppc (an int or a range) particles each, shuffled, random velocities."""
    rng = np.random.default_rng(seed)
    pos = fill_cells(rng, lo3, hi3, ppc)
    pos = pos[rng.permutation(len(pos))]
    return n, pos, rng.standard_normal(pos.shape), None


def reuse_scenes(n=96):
    """The particle sets of the one-handle sequence (test_gpu_p2g.test_one_handle_many_calls): name -> builder."""
    lo, hi = bounds(n)
    big = lambda: block(n, [-12, -12, lo + 2], [11, 11, hi - 2], (1, 24), 1)

    def holed():
        # the big box again, but a 7 x 7 bundle of columns has lost everything from z = -1 up: with the box's z pieces
        # (index 1 .. 47 and 48 .. 94 at n = 96, i.e. the upper one from coordinate 0) the inner columns' upper pieces
        # received particles in the call before and receive nothing now, while their neighbours still do
        _, pos, vel, _ = big()
        b = c_round(pos)
        gone = (np.abs(b[:, 0]) <= 3) & (np.abs(b[:, 1]) <= 3) & (b[:, 2] >= -1)
        return n, pos[~gone], vel[~gone], None

    def piled():
        _, pos, vel, _ = block(n, [-6, -6, -20], [5, 5, 19], 3, 7)
        rng = np.random.default_rng(8)
        heaps = [np.array(c, dtype=np.float64) + rng.uniform(-0.49, 0.49, size=(k, 3))
                 for c, k in (((0, 0, 0), 700), ((-3, 2, 25), 300), ((lo + 2, 0, 0), 1500), ((4, hi - 2, -30), 513))]
        pos = np.concatenate([pos] + heaps)
        return n, pos, np.concatenate([vel, rng.standard_normal((len(pos) - len(vel), 3))]), None
    return {
        "big": big,
        "small_inside": lambda: block(n, [-3, -3, -3], [2, 2, 2], (4, 30), 2),
        "small_far": lambda: block(n, [hi - 8, lo + 3, hi - 9], [hi - 3, lo + 7, hi - 4], (4, 30), 3),
        "empty": lambda: (n, np.zeros((0, 3)), np.zeros((0, 3)), None),
        "holed": holed,
        "wider": lambda: block(n, [-30, -30, lo + 2], [29, 29, hi - 2], 3, 4),   # more particles and a larger box: every buffer of the call grows
        "piled": piled,
    }


def heaped(n=96, heap=20000):
    """Thin water in a wide, flat box (58 x 58 columns, one z piece) with heaps of `heap` particles in three cells: the
    regular y segments of the row form hold several columns, and those around a heap more particles than a work item's budget,
    so the work list cuts them further."""
    lo, hi = bounds(n)
    _, pos, vel, _ = block(n, [-29, -29, -10], [28, 28, 9], 1, 21)
    rng = np.random.default_rng(22)
    heaps = [np.array(c, dtype=np.float64) + rng.uniform(-0.49, 0.49, size=(k, 3))
             for c, k in (((0, 0, 0), heap), ((-29, 17, 5), heap // 2 + 1), ((20, -28, -9), heap + 1))]
    pos = np.concatenate([pos] + heaps)
    o = rng.permutation(len(pos))
    return n, pos[o], np.concatenate([vel, rng.standard_normal((len(pos) - len(vel), 3))])[o], None


def dense_slab(n=96, ppc=(16, 17), seed=13, unit_velocity=False):
    """At n = 96: 88 x 88 columns of 58 cells, every cell with ppc[0] .. ppc[1] particles (7 M particles): the regular y segments of the
    row form hold 9 columns of full rows, more than a work item's budget of 8192 particles with no heap anywhere, so every
    segment is cut further.  16-17: no cell crowded; 18-19: every cell crowded."""
    lo, hi = bounds(n)
    rng = np.random.default_rng(seed)
    pos = fill_cells(rng, [lo + 4, lo + 4, max(-29, lo + 3)], [hi - 4, hi - 4, min(28, hi - 3)], ppc)
    pos = pos[rng.permutation(len(pos))]
    vel = np.ones_like(pos) if unit_velocity else rng.standard_normal(pos.shape)
    return n, pos, vel, None


# ---- the row form's work decomposition, restated from its documentation ----------------------------------------------------
# (comments above k_p2g_rows, k_p2g_items, k_p2g_combine and p2g_cut in csrc/kernels_particles.hip).  The tests use it only to
# show that a scene reaches a path (a segment cut by the budget, a column piece fed by nothing), never to predict a value.
P2G_ZT, P2G_BUDGET, P2G_SLOTS = 62, 8192, 1024


def box_of(n, pos):
    """The active box of a call: the base cells' bounding box, one cell wider, clipped to the grid ((lo3, hi3) in index
    space, as stats()["box_lo"], ["box_hi"]); None if no particle is on the grid."""
    lo = -(n // 2)
    b = c_round(np.asarray(pos, dtype=np.float64).reshape(-1, 3)) - lo
    on = np.all((b >= 0) & (b < n), axis=1)
    if not on.any():
        return None
    b = b[on].astype(np.int64)
    return np.maximum(b.min(0) - 1, 0).tolist(), np.minimum(b.max(0) + 1, n - 1).tolist()


def launch_cut(box):
    """(ntz, zt, nseg): z is cut into equal pieces of at most 62 target cells; y into the number of segments with the
    shortest estimated makespan (a segment of ys columns costs ys + 2 staged rows, blocks run 1024 at a time)."""
    (x0, y0, z0), (x1, y1, z1) = box
    nx, ny, nz = x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1
    ntz = (nz + P2G_ZT - 1) // P2G_ZT
    zt = (nz + ntz - 1) // ntz
    per = (nx + 2) * ntz
    best, nseg = None, 1
    for k in range(1, ny + 1):
        cost = ((per * k + P2G_SLOTS - 1) // P2G_SLOTS) * ((ny + k - 1) // k + 2)
        if best is None or cost < best:
            best, nseg = cost, k
    return ntz, zt, nseg


def _base_counts(n, pos):
    lo = -(n // 2)
    b = c_round(np.asarray(pos, dtype=np.float64).reshape(-1, 3)) - lo
    b = b[np.all((b >= 0) & (b < n), axis=1)].astype(np.int64)
    h = np.zeros((n, n, n), dtype=np.int64)
    np.add.at(h, (b[:, 0], b[:, 1], b[:, 2]), 1)
    return h


def work_items(n, pos, box):
    """Per (source x-plane, regular y segment): (columns in the segment, particles in its rows Y0-1 .. Y1+1, pieces it is cut
    into).  A segment is cut into ceil(particles / (8192 * ntz)) pieces, at most one per column."""
    (x0, y0, z0), (x1, y1, z1) = box
    ny = y1 - y0 + 1
    ntz, zt, nseg = launch_cut(box)
    rows = _base_counts(n, pos).sum(axis=2)          # particles per (x, y) row
    out = []
    for rx in range(max(x0 - 1, 0), min(x1 + 1, n - 1) + 1):
        for sy in range(nseg):
            Y0, Y1 = y0 + sy * ny // nseg, y0 + (sy + 1) * ny // nseg - 1
            c = int(rows[rx, max(Y0 - 1, 0):min(Y1 + 1, n - 1) + 1].sum())
            ln = Y1 - Y0 + 1
            nsub = min(max(-(-c // (P2G_BUDGET * ntz)), 1), ln)
            out.append((ln, c, nsub))
    return out


def fed_pieces(n, pos, box):
    """Which column pieces receive anything: a bool array [3 source x-planes (X - 1, X, X + 1)][X][y][z piece] over the box.
    Piece tz of column (X, y) is fed from plane rx iff a particle has its base cell in plane rx, rows y - 1 .. y + 1 and the
    piece's z range widened by one cell.  Pieces fed by nothing are flagged instead of written (k_p2g_combine)."""
    (x0, y0, z0), (x1, y1, z1) = box
    nx, ny = x1 - x0 + 1, y1 - y0 + 1
    ntz, zt, _ = launch_cut(box)
    occ = _base_counts(n, pos) > 0
    fed = np.zeros((3, nx, ny, ntz), dtype=bool)
    for tz in range(ntz):
        za, zb = max(z0 + tz * zt - 1, 0), min(z0 + tz * zt + zt, n - 1)
        col = occ[:, :, za:zb + 1].any(axis=2)       # (x, y): a particle in this row and z range
        for e in range(3):
            for X in range(x0, x1 + 1):
                rx = X - 1 + e
                if 0 <= rx < n:
                    for y in range(y0, y1 + 1):
                        fed[e, X - x0, y - y0, tz] = col[rx, max(y - 1, 0):min(y + 1, n - 1) + 1].any()
    return fed


def cpu_families():
    """The scene families of the GPU tests at sizes a CPU test affords (n <= 64): name -> builder."""
    return {
        "water24": lambda: water(24, 4, seed=1),
        "water33": lambda: water(33, 3, seed=2),
        "water64_full_z": lambda: water(64, 2, seed=64, full_z=True),
        "water32_unit_velocity": lambda: water(32, 8, seed=3, unit_velocity=True),
        "piles1": lambda: piles(1), "piles2": lambda: piles(2), "piles3": lambda: piles(3),
        "thresholds": thresholds,
        "edges": edges,
        "dense_rows_16_17": lambda: dense_rows(20, (16, 17)),
        "dense_rows_18_19": lambda: dense_rows(20, (18, 19), unit_velocity=True),
        "on_centres": lambda: on_centres(24, most=3000),
        "ties": ties,
        "grazing_water": lambda: grazing("water"),
        "tall64": lambda: tall_water(64),
        "tall33_unit_velocity": lambda: tall_water(33, seed=5, unit_velocity=True),
        "reuse_small_inside": lambda: reuse_scenes(64)["small_inside"](),
        "reuse_small_far": lambda: reuse_scenes(64)["small_far"](),
        "reuse_big": lambda: reuse_scenes(64)["big"](),
        "reuse_holed": lambda: reuse_scenes(64)["holed"](),
        "reuse_piled": lambda: reuse_scenes(64)["piled"](),
        "reuse_wider": lambda: block(64, [-20, -20, -30], [19, 19, 29], 3, 4),
        "heaped": lambda: heaped(64, heap=9000),
        "dense_slab": lambda: dense_slab(32),
        "one": lambda: (24, np.array([[0.3, 2.2, -1.7]]), np.full((1, 3), 0.5), None),
        "empty": lambda: (24, np.zeros((0, 3)), np.zeros((0, 3)), None),
        "all_off_grid": lambda: (24, np.array([[14.5, 0, 0], [0, -15.0, 0], [1e6, 1e6, -1e6], [0, 0, 12.2]]), np.full((4, 3), 0.5), None),
    }
