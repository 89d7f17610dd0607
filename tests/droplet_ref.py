"""Plain numpy reference for the droplet search and the per-droplet solve (csrc/kernels_droplets.hip).  No GPU, not a conftest:
tests import it.

Three things live here:

  label / claim_rule   the 6-connected components of the unknowns, and the contract of the kernel's header comment restated from
                       its TEXT (not from the kernel's code): which components must leave the global solve, which must not;
  pocket_cg            the Jacobi-preconditioned CG of ConjugateGradient.h:28-90 in float64 on one pocket's own matrix;
  SCENES               hand-built masks, one builder per edge of the contract.  Each returns (container float32 n^3,
                       solid uint8 n^3, notes); notes["pockets"] lists every hand pocket with its expected verdict written out.

Where the cores lie.  A field uploaded through fluid_upload_field widens the solver box to the whole grid (fluid_api.hip, end of
fluid_upload_field: Rb = {0 .. n-1}^3), so make_lbox gives x0 = y0 = z0 = 0 and local (i, j, k) = (x + 1, y + 1, z + LBOX_K0).
k_drop_find's block (bx, by, bz) has its 8^3 core at local (1 + 8 bx, 1 + 8 by, LBOX_K0 + 8 bz), i.e. at GRID coordinates
(8 bx, 8 by, 8 bz): the cores start at multiples of 8 on every axis, the 16^3 window of a core with origin o covers o-4 .. o+11.
The builders place pockets by `core` and core-relative `rel` coordinates: cell = 8 core + rel.

The grid: cells outside W = [2, n-3]^3 are solid (fluid_set_solid demands it), y is up, the flat index is (x n + y) n + z.  An
"unknown" is a non-solid fluid cell with at least one non-solid neighbour (pressure_system.restate: count > 0).

Out of scope: a pocket sealed in solid on ALL sides is a singular block (pure Neumann); no scene contains one — the sealed pockets
keep one open face.
"""
from collections import deque

import numpy as np

import pressure_system as ps

POCKET_MAX = 64      # cells a claimed component may have
REACH = 10           # DROP_MAXSWEEPS: cells a pocket may reach from its first cell (path length inside the pocket)
CORE = 8
DROP_CAP = 65536
DROP_NCTR = 64
CG_TOL = 2.220446049250313e-16   # fluid_default_params: cg_tol
def drop_solve_cap(n):
    """k_drop_solve's iteration cap for a pocket of n cells (restated; see the counts next to its loop)."""
    return 2 * n + 16


DT_REF = 0.1                     # fluid_default_params: max_dt, the dt of a fresh handle (scales A uniformly)


# ---------------------------------------------------------------------------------------------------------------- labelling
def unknown_mask(container, solid):
    """Non-solid fluid cells with a non-zero neighbour count (n, n, n) bool."""
    c = np.asarray(container)
    n = c.shape[0]
    free = np.asarray(solid).reshape(n, n, n) == 0
    fluid = (c.reshape(n, n, n) > 0) & free
    cnt = np.zeros((n, n, n), dtype=np.int64)
    cnt[1:] += free[:-1]; cnt[:-1] += free[1:]
    cnt[:, 1:] += free[:, :-1]; cnt[:, :-1] += free[:, 1:]
    cnt[:, :, 1:] += free[:, :, :-1]; cnt[:, :, :-1] += free[:, :, 1:]
    return fluid & (cnt > 0)


class Components:
    """ids: component per cell (n^3 flat, -1 off the unknowns), numbered by first cell; sizes; first: lowest flat index of each;
    cells: one ascending flat-index array per component."""

    def __init__(self, n, ids, sizes, first, cells):
        self.n, self.ids, self.sizes, self.first, self.cells = n, ids, sizes, first, cells

    def __len__(self):
        return len(self.sizes)


def label(unknown):
    """6-connected components by a plain breadth-first search from every unvisited unknown in index order."""
    unknown = np.asarray(unknown, dtype=bool)
    n = unknown.shape[0]
    assert unknown.shape == (n, n, n)
    assert not (unknown[0].any() or unknown[-1].any() or unknown[:, 0].any() or unknown[:, -1].any() or unknown[:, :, 0].any()
                or unknown[:, :, -1].any()), "an unknown on the grid's outer layer"
    flat = unknown.reshape(-1)
    ids = np.full(n ** 3, -1, dtype=np.int64)
    todo = flat.tolist()
    out = ids.tolist()
    strides = (n * n, -n * n, n, -n, 1, -1)
    sizes, first, cells = [], [], []
    for start in np.flatnonzero(flat).tolist():
        if out[start] >= 0:
            continue
        c = len(sizes)
        out[start] = c
        mine = [start]
        q = deque(mine)
        while q:
            a = q.popleft()
            for s in strides:
                b = a + s
                if todo[b] and out[b] < 0:
                    out[b] = c
                    mine.append(b)
                    q.append(b)
        mine.sort()
        sizes.append(len(mine))
        first.append(mine[0])
        cells.append(np.array(mine, dtype=np.int64))
    return Components(n, np.array(out, dtype=np.int64), np.array(sizes, dtype=np.int64), np.array(first, dtype=np.int64), cells)


def _eccentricity(cells, start, n, limit):
    """Largest path length inside the cell set from `start` (stops counting past `limit`)."""
    inside = set(cells)
    dist = {start: 0}
    q = deque([start])
    far = 0
    strides = (n * n, -n * n, n, -n, 1, -1)
    while q:
        a = q.popleft()
        for s in strides:
            b = a + s
            if b in inside and b not in dist:
                dist[b] = dist[a] + 1
                far = max(far, dist[b])
                if far > limit:
                    return far
                q.append(b)
    assert len(dist) == len(inside)
    return far


def claim_rule(comps, n, own=None):
    """The header comment of kernels_droplets.hip as a predicate per component (bool array): a component MUST be claimed when
      - it has at most 64 cells,
      - every cell is within 10 cells (path length inside the component) of its first cell,
      - with o = the first cell's coordinates rounded down to multiples of 8 (the origin of the one core that owns it), every
        cell lies in o-3 .. o+10 on every axis: inside the 16^3 window o-4 .. o+11 with a free layer around it,
      - every cell lies in `own` (bool, n^3; a decomposed rank's owned cells), when given;
    and must NOT be claimed when any clause fails."""
    own = None if own is None else np.asarray(own, dtype=bool).reshape(-1)
    verdict = np.zeros(len(comps), dtype=bool)
    for c in range(len(comps)):
        cells = comps.cells[c]
        if len(cells) > POCKET_MAX:
            continue
        x, r = np.divmod(cells, n * n)
        y, z = np.divmod(r, n)
        f = int(comps.first[c])
        o = np.array([f // (n * n), (f // n) % n, f % n]) // CORE * CORE
        rel = np.stack([x, y, z], axis=1) - o
        if rel.min() < -3 or rel.max() > CORE + 2:
            continue
        if own is not None and not own[cells].all():
            continue
        if len(cells) > 1 and _eccentricity(cells.tolist(), f, n, REACH) > REACH:
            continue
        verdict[c] = True
    return verdict


# ------------------------------------------------------------------------------------------------------------ the matrix, CG
def restate_masks(container, solid, dt=DT_REF):
    """pressure_system.System of a mask pair: the unknowns numbered in index order like the device's scan."""
    c = np.asarray(container)
    n = c.shape[0]
    s = np.asarray(solid).reshape(-1)
    fluid = (c.reshape(-1) > 0) & (s == 0)
    idx = np.full(n ** 3, -1, dtype=np.int64)
    idx[fluid] = np.arange(int(fluid.sum()))
    return ps.restate(s, c.reshape(-1), idx, dt)


def pocket_matrix(sys_, rows):
    """The dense block of the rows `rows` (a closed pocket: no entry leaves it)."""
    rows = np.asarray(rows, dtype=np.int64)
    pos = {int(r): i for i, r in enumerate(rows)}
    A = np.zeros((len(rows), len(rows)))
    for i, r in enumerate(rows):
        A[i, i] = sys_.diag[r]
        for d in range(6):
            j = int(sys_.nb[r, d])
            if j >= 0:
                assert j in pos, "the rows are not a closed pocket"
                A[i, pos[j]] = sys_.off
    return A


def pocket_cg(A, b, tol=CG_TOL, cap=None):
    """ConjugateGradient.h:28-90 with the diagonal preconditioner, x0 = 0, float64.  Stops when |r|^2 <= tol^2 |b|^2 (the
    recursive residual) or after `cap` iterations.  Returns (x, iterations, sqrt(|r|^2 / |b|^2))."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    inv = 1.0 / np.diag(A)
    x = np.zeros_like(b)
    bb = float(b @ b)
    if bb == 0:
        return x, 0, 0.0
    thr = tol * tol * bb
    r = b.copy()
    p = inv * r
    rz = float(r @ p)
    rr = bb
    it = 0
    while rr > thr and (cap is None or it < cap):
        q = A @ p
        alpha = rz / float(p @ q)
        x += alpha * p
        r -= alpha * q
        rr = float(r @ r)
        it += 1
        if rr <= thr:
            break
        z = inv * r
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
        assert it < 100 * len(b) + 100, "the reference CG does not converge"
    return x, it, float(np.sqrt(rr / bb))


# ------------------------------------------------------------------------------------------------------------------- scenes
def shell_solid(n):
    s = np.ones((n, n, n), dtype=np.uint8)
    s[2:n - 2, 2:n - 2, 2:n - 2] = 0
    return s


def at(core, rel):
    return tuple(CORE * c + r for c, r in zip(core, rel))


def box(o, size):
    sx, sy, sz = (size,) * 3 if np.isscalar(size) else size
    return [(o[0] + i, o[1] + j, o[2] + k) for i in range(sx) for j in range(sy) for k in range(sz)]


def line(o, axis, length):
    return [tuple(o[a] + (q if a == axis else 0) for a in range(3)) for q in range(length)]


def path(o, moves):
    """Cells of a walk from o: moves = [(axis, signed steps), ...]."""
    cells, p = [tuple(o)], list(o)
    for axis, steps in moves:
        for _ in range(abs(steps)):
            p[axis] += 1 if steps > 0 else -1
            cells.append(tuple(p))
    return cells


POOL = (slice(4, 28), slice(2, 4), slice(4, 16))   # 24 x 2 x 12 = 576 cells on the floor: the global solve is not empty


class _Scene:
    def __init__(self, n=48, pool=True):
        self.n = n
        self.c = np.zeros((n, n, n), dtype=np.float32)
        self.s = shell_solid(n)
        self.pockets = []
        self.extra = {}
        if pool:
            self.c[POOL] = 1.0

    def seal(self, lo, hi):
        """Solid over the inclusive box lo .. hi (pockets are carved out of it afterwards)."""
        self.s[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = 1

    def open(self, cell):
        self.s[cell] = 0

    def pocket(self, name, cells, claim, why, joined=False, sealed=False):
        """claim: the verdict the contract gives this pocket.  joined: the cells hang on another component on purpose."""
        n = self.n
        for c in cells:
            assert all(2 <= v <= n - 3 for v in c), (name, c)
            assert self.c[c] == 0, (name, c, "cell used twice")
            self.c[c] = 1.0
            self.s[c] = 0
        flat = np.sort(np.array([(c[0] * n + c[1]) * n + c[2] for c in cells], dtype=np.int64))
        self.pockets.append(dict(name=name, cells=flat, claim=claim, why=why, joined=joined, sealed=sealed))

    def done(self, **extra):
        notes = dict(n=self.n, pockets=self.pockets, overflow=False)
        notes.update(self.extra)
        notes.update(extra)
        return self.c, self.s, notes


def scene_size():
    s = _Scene()
    s.pocket("cube 4x4x4 (64)", box(at((1, 2, 1), (2, 2, 2)), 4), True, "64 cells is the largest claim; corner to corner is 9")
    s.pocket("cube + 1 (65)", box(at((3, 2, 1), (2, 2, 2)), 4) + [at((3, 2, 1), (6, 5, 5))], False, "65 cells")
    c63 = box(at((1, 2, 3), (2, 2, 2)), 4)
    c63.remove(at((1, 2, 3), (5, 5, 5)))
    s.pocket("cube - 1 (63)", c63, True, "63 cells")
    return s.done()


def scene_reach_lines():
    s = _Scene()
    s.pocket("line 11 +x", line(at((1, 2, 1), (0, 3, 3)), 0, 11), True, "last cell 10 from the first, at o+10")
    s.pocket("line 12 +x", line(at((1, 2, 3), (0, 3, 3)), 0, 12), False, "last cell 11 from the first (and at o+11)")
    s.pocket("line 11 +y", line(at((3, 1, 1), (3, 0, 3)), 1, 11), True, "as +x")
    s.pocket("line 12 +y", line(at((3, 1, 3), (3, 0, 3)), 1, 12), False, "as +x")
    s.pocket("line 11 +z", line(at((1, 4, 1), (3, 3, 0)), 2, 11), True, "as +x")
    s.pocket("line 12 +z", line(at((3, 4, 1), (3, 3, 0)), 2, 12), False, "as +x")
    return s.done()


def _hook(o, last):
    return path(o, [(2, 5), (1, 3), (2, -last)])       # first cell = the tip: lowest y of its x, lowest z of that row


def _c_shape(o, k, extra):
    """Two arms along +y at x and x+2 joined at their tops: both arm ends are local first cells (no unknown before them on any
    axis).  The lower one (the component's first cell) is k + 2 + k + extra cells from the other arm's end."""
    x, y, z = o
    return line(o, 1, k + 1) + [(x + 1, y + k, z)] + line((x + 2, y - extra, z), 1, k + 1 + extra)


def scene_reach_bent():
    s = _Scene()
    s.pocket("hook 10", _hook(at((1, 2, 1), (3, 2, 1)), 2), True, "path length 10 from the tip, inside a 1 x 4 x 6 box")
    s.pocket("hook 11", _hook(at((3, 2, 1), (3, 2, 1)), 3), False, "path length 11, same box: reach alone decides")
    s.pocket("C 10", _c_shape(at((1, 2, 3), (2, 3, 3)), 4, 0), True, "two local first cells; the lower label needs 10 sweeps")
    s.pocket("C 11", _c_shape(at((3, 2, 3), (2, 3, 3)), 4, 1), False, "the lower label needs 11")
    return s.done()


def scene_window():
    s = _Scene()
    s.pocket("first cell at core (0,0,0)", box(at((1, 1, 1), (0, 0, 0)), 2), True, "core corner")
    s.pocket("first cell at core (7,7,7)", box(at((1, 1, 3), (7, 7, 7)), 2), True, "core corner, cells at o+7 .. o+8")
    for axis, name, cores, rel in ((0, "x", ((3, 1, 1), (3, 1, 3)), (7, 3, 3)), (1, "y", ((1, 3, 1), (1, 3, 3)), (3, 7, 3)),
                                   (2, "z", ((3, 3, 1), (3, 3, 3)), (3, 3, 7))):
        s.pocket(f"{name} up to o+10", line(at(cores[0], rel), axis, 4), True, "last layer inside the free layer")
        s.pocket(f"{name} up to o+11", line(at(cores[1], rel), axis, 5), False, "a cell on the window's outer layer (5 cells, reach 4)")
    return s.done()


def scene_window_low():
    """Cells below the core on y and z exist only at a larger x than the first cell's."""
    s = _Scene()
    s.pocket("y down to o-3", path(at((2, 2, 1), (2, 0, 3)), [(0, 1), (1, -3)]), True, "o-3 is inside the free layer")
    s.pocket("y down to o-4", path(at((2, 2, 3), (2, 0, 3)), [(0, 1), (1, -4)]), False, "o-4 is the window's outer layer")
    s.pocket("z down to o-3", path(at((2, 4, 2), (2, 3, 0)), [(0, 1), (2, -3)]), True, "as y")
    s.pocket("z down to o-4", path(at((4, 4, 2), (2, 3, 0)), [(0, 1), (2, -4)]), False, "as y")
    return s.done()


def scene_neighbours():
    s = _Scene()
    s.pocket("edge pair A", box(at((1, 2, 1), (1, 1, 1)), 2), True, "touches B along an edge only")
    s.pocket("edge pair B", box(at((1, 2, 1), (3, 3, 1)), 2), True, "touches A along an edge only")
    s.pocket("corner pair A", box(at((3, 2, 1), (1, 1, 1)), 2), True, "touches B at a corner only")
    s.pocket("corner pair B", box(at((3, 2, 1), (3, 3, 3)), 2), True, "touches A at a corner only")
    s.pocket("gap pair A", box(at((1, 2, 3), (1, 1, 1)), 2), True, "one air cell from B, same window")
    s.pocket("gap pair B", box(at((1, 2, 3), (4, 1, 1)), 2), True, "one air cell from A, same window")
    s.pocket("above the pool", box((8, 5, 8), 2), True, "one air cell above the pool")
    s.pocket("on the pool", box((16, 5, 8), 2) + [(16, 4, 8)], False, "joined to the pool by one face: part of the pool", joined=True)
    s.seal((35, 29, 35), (37, 31, 37))
    s.c[36, 30, 36] = 1.0
    s.open((36, 30, 36))
    return s.done(walled=[(36 * 48 + 30) * 48 + 36])   # fluid, six solid neighbours: not an unknown, p = 0


def scene_crowd():
    s = _Scene()
    o = at((2, 3, 2), (0, 0, 0))
    for c in box(o, 8):
        if (c[0] + c[1] + c[2]) % 2 == 0:
            s.pocket(f"single {c}", [c], True, "a single cell: p = b / diag")
    assert len(s.pockets) == 256
    return s.done()


def scene_overflow():
    """n = 64: single cells on a 3-D checkerboard over all of W.  60^3 / 2 = 108 000 pockets > DROP_CAP; the 8 blocks that share a
    counter (blockIdx % 64) claim 6 * 256 + 2 * 192 = 1 920 > 1 024 in every range whose blocks lie inside W on y and z."""
    n = 64
    s = _Scene(n, pool=False)
    i = np.arange(n)
    board = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0) & (s.s == 0)
    s.c[board] = 1.0
    return s.done(overflow=True)


def _three(s):
    s.pocket("box", box(at((1, 2, 1), (2, 2, 2)), 2), True, "2 x 2 x 2")
    s.pocket("line 5", line(at((3, 2, 1), (1, 3, 3)), 2, 5), True, "1 x 1 x 5")
    s.pocket("L", path(at((1, 2, 3), (2, 2, 2)), [(0, 2), (1, 2)]), True, "bent")


def scene_three():
    s = _Scene()
    _three(s)
    return s.done()


def scene_all_pockets():
    s = _Scene(pool=False)
    _three(s)
    return s.done()


def scene_none():
    return _Scene().done()


def scene_solids():
    s = _Scene()
    s.seal((10, 20, 10), (37, 21, 37))                  # a shelf two cells thick in mid air
    s.pocket("on the shelf", box((12, 22, 12), 2), True, "solid below")
    s.pocket("on the shelf 2", box((30, 22, 20), (3, 1, 2)), True, "solid below")
    s.pocket("under the shelf", box((20, 18, 30), 2), True, "solid above")
    s.pocket("at the x wall", box((2, 30, 20), 2), True, "solid at x - 1")
    s.pocket("in the corner", box((2, 44, 2), 2), True, "three walls")
    return s.done()


def _comb(o):
    x, y, z = o
    cells = line(o, 2, 11)                                            # spine along +z: o .. o+10
    for q, length in ((0, 4), (2, 4), (4, 4), (6, 4), (8, 2)):        # teeth along +x, tip at most 10 from the first cell
        cells += line((x + 1, y, z + q), 0, length)
    for q in (1, 3, 5, 7):                                            # teeth along +y
        cells += line((x, y + 1, z + q), 1, 3)
    assert len(cells) == 41
    return cells


def scene_sealed():
    """Pockets cast in solid with one open face (one air cell): Neumann everywhere else, Jacobi-scaled condition 200 - 900."""
    s = _Scene()
    s.seal((7, 26, 10), (19, 28, 12))
    s.pocket("sealed line 11", line(at((1, 3, 1), (0, 3, 3)), 0, 11), True, "11 cells, open at its far end", sealed=True)
    s.open((19, 27, 11))
    o = at((3, 3, 2), (0, 2, 0))
    s.seal((o[0] - 1, o[1] - 1, o[2] - 1), (o[0] + 5, o[1] + 4, o[2] + 11))
    s.pocket("sealed comb 41", _comb(o), True, "41 cells within reach 10, open at the spine's far end", sealed=True)
    s.open((o[0], o[1], o[2] + 11))
    s.seal((9, 9, 25), (14, 14, 30))
    s.pocket("sealed cube 64", box((10, 10, 26), 4), True, "64 cells, one cell's face open", sealed=True)
    s.open((13, 13, 30))
    s.seal((7, 7, 7), (19, 19, 19))
    s.pocket("sealed fan 3 x 10", line((8, 8, 8), 0, 11) + line((8, 9, 8), 1, 10) + line((8, 8, 9), 2, 10), True,
             "31 cells: arms of 10 along +x, +y, +z from the first cell, open at the +x tip", sealed=True)
    s.open((19, 8, 8))
    s.seal((31, 7, 7), (33, 19, 19))
    s.pocket("sealed V 2 x 10", line((32, 8, 8), 1, 11) + line((32, 8, 9), 2, 10), True,
             "21 cells: a path with the first cell in its middle, open at the +y tip", sealed=True)
    s.open((32, 19, 8))
    return s.done()


def scene_grid_edge():
    """n = 44 is no multiple of 8: the last core block on each axis (40 .. 47) holds two layers of W (40, 41) and the wall."""
    s = _Scene(44)
    s.pocket("last x block", box((40, 20, 20), 2), True, "first cell in the partial block on x")
    s.pocket("last y block", box((20, 40, 20), 2), True, "... on y")
    s.pocket("last z block", box((20, 20, 40), 2), True, "... on z")
    s.pocket("last block of all", box((40, 40, 40), 2), True, "... on all three")
    return s.done()


SCENES = {
    "size": scene_size, "reach_lines": scene_reach_lines, "reach_bent": scene_reach_bent, "window": scene_window,
    "window_low": scene_window_low, "neighbours": scene_neighbours, "crowd": scene_crowd, "overflow": scene_overflow,
    "three": scene_three, "all_pockets": scene_all_pockets, "none": scene_none, "solids": scene_solids, "sealed": scene_sealed,
    "grid_edge": scene_grid_edge,
}


_BUILT = {}


def built(name):
    """(container, solid, notes, components, system) of a scene: built once, shared between tests, never changed."""
    if name not in _BUILT:
        c, s, notes = SCENES[name]()
        for a in (c, s):
            a.setflags(write=False)
        _BUILT[name] = (c, s, notes, label(unknown_mask(c, s)), restate_masks(c, s))
    return _BUILT[name]


def expected_claims(comps, notes):
    """The hand verdicts mapped onto the labelling: (component -> verdict) for every component that is a hand pocket, after
    checking that each unjoined hand pocket IS one whole component."""
    out = {}
    for p in notes["pockets"]:
        c = int(comps.ids[p["cells"][0]])
        assert c >= 0, p["name"]
        if p["joined"]:
            assert comps.sizes[c] > POCKET_MAX and (comps.ids[p["cells"]] == c).all() and not p["claim"], p["name"]
        else:
            assert np.array_equal(comps.cells[c], p["cells"]), f"{p['name']}: not a component of its own"
            out[c] = p["claim"]
    return out


def particles_on_centres(container, lo):
    """One particle on the centre of every fluid cell of the mask: coordinates lo + index (grid_bounds)."""
    c = np.asarray(container)
    return np.argwhere(c > 0).astype(np.float64) + float(lo)


def scene_decomposed():
    """n = 48 for 2 x 2 x 2 blocks cut at index 24 on every axis.  Only 2 x 2 x 2 and 2 x 1 x 1 pockets: their verdict does not
    depend on where a rank's cores start (a rank's solver box has its own origin), only on the owned cells."""
    s = _Scene()                                      # (the pool lies across the x cut)
    s.pocket("inside a block", box((10, 30, 10), 2), True, "its 16^3 window lies inside the owner's cells")
    s.pocket("owned, window into the halo", box((21, 30, 10), 2), True, "all cells below the cut at 24, the window crosses it")
    s.pocket("owned on the far side", box((24, 30, 40), 2), True, "first cell on the cut's upper side, the window crosses it")
    s.pocket("across the x cut", [(23, 30, 34), (24, 30, 34)], False, "one cell on each side: stays in the global solve")
    s.pocket("across the z cut", [(36, 36, 23), (36, 36, 24)], False, "as x")
    s.pocket("on the corner of three cuts", box((23, 23, 23), 2), False, "one cell in each of the eight blocks")
    return s.done(cuts=24)                            # the verdicts are those of the decomposed run


def block_masks(n, cut):
    """The owned cells of each of the 2 x 2 x 2 blocks cut at index `cut` (bool n^3 each)."""
    out = []
    for bx in range(2):
        for by in range(2):
            for bz in range(2):
                m = np.zeros((n, n, n), dtype=bool)
                m[tuple(slice(0, cut) if b == 0 else slice(cut, n) for b in (bx, by, bz))] = True
                out.append(m)
    return out


DECOMPOSED = "decomposed"
SCENES[DECOMPOSED] = scene_decomposed
