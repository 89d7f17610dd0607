"""The two V-cycles that precondition the pressure solve, restated in plain numpy on whole arrays: z = M^-1 b.

Not a conftest: tests import it.  Written from the design as kernels_mg.hip and kernels_gal.hip state it in their headers, mg_coef /
make_coef (fluid_api.hip) and the defaults of sim.h; there are no tiles, no halos and no launches here.  Every function takes the
arithmetic dtype (float32, float64, longdouble), so the reference can measure its own rounding: the bars of tests/test_gpu_vcycle.py
are differences between two runs of this file.

A level is a dx x dy x dz array of cell types: 0 solid (and everything off the domain), 1 air (p = 0), 2 unknown.  Level 0 is the
solver's active box plus a ring of one cell; a coarser level has (d + 1) / 2 cells per axis, anchored at cell 0, until every axis is <= 8
(at least two levels).

Re-discretised cycle (kernels_mg.hip): a coarse cell is air if any child is air, solid if all are solid, else an unknown; its row is the
7-point form with off-diagonal -scale / 4^l and diagonal (non-solid neighbours) x scale / 4^l.  Level 0 keeps the reference's own
float-accumulated diagonal table and off = float(-scale) (tests/pressure_system.py).  Damped Jacobi from u = 0 with (W1, W2) before the
coarse correction and (W2, W1) after it; restriction P^T / 8 with cell-centred trilinear P, written to unknown coarse cells only; the
correction weighted by `wc` of the level it goes into; the coarsest level by symmetric red-black Gauss-Seidel.  The weight of a correction
depends on where the level runs (kernels_mg.hip:33-34, sim.h mg_wc: "level 0 / level 1 / deeper kernel levels / inside the tail"): 1.25
into level 0, 1.1 into level 1, 1 deeper AND into every level that the one-block tail kernel holds — so a level 1 inside the tail takes 1,
not 1.1.  plan() restates mg_setup's choice of the first tail level; nothing else here knows about the tail.

Galerkin cycle (kernels_gal.hip): level 0 as above, but its coarse right-hand side is the plain sum of the residual over the 8 children
and its correction 1.8 x the parent's value.  A coarse cell is an unknown if any child is; rows are A_c = P^T A P with P piecewise
constant over the unknown children, kept as the diagonal gd and the +x / +y / +z face weights gx, gy, gz.  Sweeps (0.5617, 1.6) on the
levels >= 1, (0.5617, 1.3895) on level 0.  The coarsest level is the first level >= 1 (at least level 2) whose cells plus a ring number
<= 3072; it is solved by symmetric red-black Gauss-Seidel, colour (i + j + k) & 1, 0 first.
"""
import numpy as np

MG_W1, MG_W2 = 0.5617, 1.3895
GAL_W1, GAL_W2 = 0.5617, 1.6
MG_WC = (1.25, 1.1, 1.0)      # into level 0 / level 1 / deeper levels that run as kernels
MG_WC_TAIL = 1.0              # into a level inside the tail
GAL_WC = 1.8
MG_CSWEEPS = 3
GAL_SWEEPS = 3
GAL_CMAX = 3072
MG_TAIL_MAX, MG_TAIL_Q0, MG_TAIL_LDS = 4, 4, 144 * 1024
MG_FOLD_CELLS = 200000        # a level 0 of more cells restricts with a launch of its own
P_NEAR, P_FAR = 0.75, 0.25    # cell-centred trilinear prolongation, per axis


# ---- hierarchy ---------------------------------------------------------------------------------------------------------------
def level_dims(d0):
    dims = [tuple(int(d) for d in d0)]
    while len(dims) < 2 or max(dims[-1]) > 8:
        dims.append(tuple((d + 1) // 2 for d in dims[-1]))
    assert len(dims) <= 8
    return dims


def _tail_bytes(dims, elem):
    total = 0
    for l, d in enumerate(dims):
        if d[0] * d[1] * d[2] > 1024 * (MG_TAIL_Q0 if l == 0 else 1):
            return 0
        c = (d[0] + 3) * (d[1] + 3) * (d[2] + 3)
        total += 3 * ((c * elem + 15) // 16 * 16) + (c + 15) // 16 * 16
    return total


def plan(d0, elem=4):
    """What mg_setup decides for a level-0 domain d0 and a cycle of `elem`-byte numbers: dims of every level, the first level of
    the tail, whether level 0 folds its restriction into the down leg, the weight of the correction INTO each level, and the
    coarsest level of the Galerkin cycle (None where that cycle does not apply)."""
    dims = level_dims(d0)
    nl = len(dims)

    def fits(t):
        b = _tail_bytes(dims[t:], elem) if nl - t <= MG_TAIL_MAX else 0
        return 0 < b <= MG_TAIL_LDS

    tail = nl - 1
    while tail > 1 and fits(tail - 1):
        tail -= 1
    assert fits(tail)
    wc = [MG_WC_TAIL if l >= tail else MG_WC[min(l, 2)] for l in range(nl - 1)]
    gal_fit = lambda d: (d[0] + 2) * (d[1] + 2) * (d[2] + 2) <= GAL_CMAX
    lc = 1
    while lc < nl - 1 and not gal_fit(dims[lc]):
        lc += 1
    gal_lc = lc if (gal_fit(dims[lc]) and lc >= 2) else None
    return {"dims": dims, "tail": tail, "fold": dims[0][0] * dims[0][1] * dims[0][2] <= MG_FOLD_CELLS, "wc": wc, "gal_lc": gal_lc}


def level0_types(solid, fluid, lo, hi):
    """Types and neighbour counts of level 0 for the active box lo..hi (inclusive, grid cells): the box plus a ring of one cell, so
    domain cell i is grid cell lo - 1 + i.  An unknown is a non-solid fluid cell with at least one non-solid neighbour."""
    solid = np.asarray(solid) != 0
    fluid = np.asarray(fluid) != 0
    n = solid.shape
    d = tuple(hi[a] - lo[a] + 3 for a in range(3))
    sol = np.ones(d, dtype=bool)
    flu = np.zeros(d, dtype=bool)
    src, dst = [], []
    for a in range(3):
        g0, g1 = max(lo[a] - 1, 0), min(hi[a] + 1, n[a] - 1)
        src.append(slice(g0, g1 + 1))
        dst.append(slice(g0 - (lo[a] - 1), g1 - (lo[a] - 1) + 1))
    sol[tuple(dst)] = solid[tuple(src)]
    flu[tuple(dst)] = fluid[tuple(src)]
    cnt = _count(~sol, flu & ~sol)
    typ = np.where(sol, 0, np.where(cnt > 0, 2, 1)).astype(np.uint8)
    return typ, cnt


def _count(nonsolid, unknown):
    p = np.pad(nonsolid, 1).astype(np.int64)
    n = p[:-2, 1:-1, 1:-1] + p[2:, 1:-1, 1:-1] + p[1:-1, :-2, 1:-1] + p[1:-1, 2:, 1:-1] + p[1:-1, 1:-1, :-2] + p[1:-1, 1:-1, 2:]
    return np.where(unknown, n, 0)


def _blocks(a):
    """(D, 2, D, 2, D, 2) view of `a` padded with zeros to even sizes."""
    D = tuple((x + 1) // 2 for x in a.shape)
    p = np.zeros(tuple(2 * x for x in D), dtype=a.dtype)
    p[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return p.reshape(D[0], 2, D[1], 2, D[2], 2)


def coarsen_types(t):
    b = _blocks(t)
    air = (b == 1).any(axis=(1, 3, 5))
    sol = (b == 0).all(axis=(1, 3, 5))
    return np.where(air, 1, np.where(sol, 0, 2)).astype(np.uint8)


def sum8(a):
    return _blocks(a).sum(axis=(1, 3, 5), dtype=a.dtype)


# ---- a 7-point operator with per-cell entries ----------------------------------------------------------------------------------
class Op:
    """Rows over the unknowns `mask`: diagonal gd, and -wx[i] couples cell i with cell i + 1 along x (wy, wz alike); a weight is 0
    where either side is no unknown or lies off the level."""

    def __init__(self, gd, wx, wy, wz, mask):
        self.gd, self.wx, self.wy, self.wz, self.mask = gd, wx, wy, wz, mask
        with np.errstate(divide="ignore"):
            self.inv = np.where(mask, 1 / np.where(mask, gd, 1), 0).astype(gd.dtype)

    def offdiag(self, u):
        """sum over the neighbours j of a cell of w_ij u_j"""
        o = np.zeros_like(u)
        o[:-1] += self.wx[:-1] * u[1:]
        o[1:] += self.wx[:-1] * u[:-1]
        o[:, :-1] += self.wy[:, :-1] * u[:, 1:]
        o[:, 1:] += self.wy[:, :-1] * u[:, :-1]
        o[:, :, :-1] += self.wz[:, :, :-1] * u[:, :, 1:]
        o[:, :, 1:] += self.wz[:, :, :-1] * u[:, :, :-1]
        return o

    def apply(self, u):
        return self.gd * u - self.offdiag(u)

    def dense(self):
        """(matrix over the unknowns in C order, flat cell index of every row)"""
        cells = np.flatnonzero(self.mask)
        row = np.full(self.mask.size, -1)
        row[cells] = np.arange(len(cells))
        A = np.zeros((len(cells), len(cells)), dtype=self.gd.dtype)
        A[np.arange(len(cells)), np.arange(len(cells))] = self.gd.reshape(-1)[cells]
        s = self.mask.shape
        for w, step in ((self.wx, s[1] * s[2]), (self.wy, s[2]), (self.wz, 1)):
            wf = w.reshape(-1)
            src = np.flatnonzero(wf != 0)
            A[row[src], row[src + step]] -= wf[src]
            A[row[src + step], row[src]] -= wf[src]
        return A, cells


def _face_weights(mask, w, T):
    out = []
    for a in range(3):
        m = np.zeros(mask.shape, dtype=bool)
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        m[tuple(lo)] = mask[tuple(lo)] & mask[tuple(hi)]
        out.append(np.where(m, w, 0).astype(T))
    return out


def op_level0(typ, cnt, scale, T):
    """setA's rows: the diagonal is `scale` accumulated in float32 once per non-solid neighbour, the coupling float32(-scale)."""
    from pressure_system import diag_table
    mask = typ == 2
    gd = np.where(mask, diag_table(scale)[cnt], 0).astype(T)
    w = T(np.float32(scale))
    return Op(gd, *_face_weights(mask, w, T), mask)


def op_rediscretised(typ, scale, level, T):
    mask = typ == 2
    s = T(np.float64(scale) / 4.0 ** level)
    gd = (_count(typ != 0, mask).astype(T) * s).astype(T)
    return Op(gd, *_face_weights(mask, s, T), mask)


def op_galerkin(fine, inner_factor=2):
    """P^T A P for P piecewise constant over the unknown children of every 2 x 2 x 2 block: the children's diagonals, minus each
    face between two children once per side (twice), and the faces towards the next block summed into its face weight."""
    T = fine.gd.dtype.type
    inner = np.zeros(tuple((x + 1) // 2 for x in fine.mask.shape), dtype=fine.gd.dtype)
    face = []
    for a, w in enumerate((fine.wx, fine.wy, fine.wz)):
        even = np.zeros_like(w)
        odd = np.zeros_like(w)
        se = [slice(None)] * 3
        so = [slice(None)] * 3
        se[a], so[a] = slice(0, None, 2), slice(1, None, 2)
        even[tuple(se)] = w[tuple(se)]
        odd[tuple(so)] = w[tuple(so)]
        inner = inner + sum8(even)
        face.append(sum8(odd))
    mask = sum8(fine.mask.astype(np.int64)) > 0
    gd = np.where(mask, sum8(np.where(fine.mask, fine.gd, 0).astype(fine.gd.dtype)) - T(inner_factor) * inner, 0).astype(fine.gd.dtype)
    return Op(gd, face[0], face[1], face[2], mask & (gd > 0))


def _child(a, A):
    """child a (bit 0: x, bit 1: y, bit 2: z) of every 2 x 2 x 2 block of A"""
    return _blocks(A)[:, a & 1, :, (a >> 1) & 1, :, a >> 2]


def op_galerkin_stored(fine, level0_scale=None):
    """The same rows as the solver keeps them: float32 arrays, every sum taken in float32 over the children in index order (x fastest),
    level 1 from the fine counts (level0_scale: float32(scale); the faces inside a block are counted, 2 x scale x count).  The design
    leaves the order and the precision of these sums open ("small integers x scale", kernels_gal.hip:9 — exactly that only if the
    multiples of scale were float32 numbers); in float32 a row carries up to 9e-7 of its diagonal in rounding by level 3, and a shallow
    pool's coarse operator is so weakly definite that z moves by 2e-6 of its maximum: eight times what the float32 cycle's own
    arithmetic does.  The cycle's arithmetic dtype stays the caller's: the rows are data, like the float32 table of level 0."""
    f32 = np.float32
    shape = tuple((x + 1) // 2 for x in fine.mask.shape)
    dsum, inner = np.zeros(shape, f32), np.zeros(shape, f32)
    count = np.zeros(shape, np.int64)
    face = [np.zeros(shape, f32) for _ in range(3)]
    mask = np.zeros(shape, bool)
    gd, ws = fine.gd.astype(f32), [w.astype(f32) for w in (fine.wx, fine.wy, fine.wz)]
    for a in range(8):
        u = _child(a, fine.mask)
        mask |= u
        dsum = np.where(u, dsum + _child(a, gd), dsum).astype(f32)
        for ax in range(3):
            c = _child(a, ws[ax])
            if not a & (1 << ax):
                inner = np.where(u, inner + c, inner).astype(f32)
                count += u & (c != 0)
            else:
                face[ax] = np.where(u, face[ax] + c, face[ax]).astype(f32)
    if level0_scale is not None:
        s = f32(level0_scale)
        inner2 = ((f32(2) * s) * count.astype(f32)).astype(f32)
        face = [(s * np.round(w.astype(np.float64) / np.float64(s)).astype(f32)).astype(f32) for w in face]
    else:
        inner2 = (f32(2) * inner).astype(f32)
    out = np.where(mask, dsum - inner2, 0).astype(f32)
    T = fine.gd.dtype
    return Op(out.astype(T), face[0].astype(T), face[1].astype(T), face[2].astype(T), mask & (out > 0))


# ---- pieces of a cycle ---------------------------------------------------------------------------------------------------------
def _pre(op, f, w1, w2, T):
    u = T(w1) * op.inv * f
    return u + T(w2) * op.inv * (f - op.apply(u))


def _sweep(op, u, f, w, T):
    return u + T(w) * op.inv * (f - op.apply(u))


def _residual(op, u, f):
    return np.where(op.mask, f - op.apply(u), 0).astype(f.dtype)


def _rbgs(op, f, sweeps, orders=((0, 1), (1, 0))):
    """symmetric red-black Gauss-Seidel from u = 0: `sweeps` times colour 0 then 1, then `sweeps` times 1 then 0"""
    i, j, k = np.indices(op.mask.shape)
    colour = (i + j + k) & 1
    u = np.zeros_like(f)
    for s in range(2 * sweeps):
        for c in orders[0 if s < sweeps else 1]:
            new = op.inv * (f + op.offdiag(u))
            u = np.where(op.mask & (colour == c), new, u).astype(f.dtype)
    return u


def _restrict_axis(r, axis, T, near, far):
    r = np.moveaxis(r, axis, 0)
    d = r.shape[0]
    D = (d + 1) // 2
    p = np.zeros((2 * D + 3,) + r.shape[1:], dtype=r.dtype)    # p[i + 1] = r[i]
    p[1:d + 1] = r
    out = T(far) * (p[0:2 * D:2] + p[3:2 * D + 3:2]) + T(near) * (p[1:2 * D + 1:2] + p[2:2 * D + 2:2])
    return np.moveaxis(out, 0, axis)


def restrict_trilinear(r, T, near=P_NEAR, far=P_FAR):
    """P^T r / 8: a coarse cell gathers the fine cells 2I - 1 .. 2I + 2 per axis with weights (far, near, near, far)"""
    for a in range(3):
        r = _restrict_axis(r, a, T, near, far)
    return r * T(0.125)


def _prolong_axis(e, d, axis, T, near, far):
    e = np.moveaxis(e, axis, 0)
    p = np.zeros((e.shape[0] + 2,) + e.shape[1:], dtype=e.dtype)    # p[I + 1] = e[I]
    p[1:-1] = e
    i = np.arange(d)
    I = i >> 1
    other = np.where(i & 1, I + 1, I - 1)
    out = T(near) * p[I + 1] + T(far) * p[other + 1]
    return np.moveaxis(out, 0, axis)


def prolong_trilinear(e, shape, T, near=P_NEAR, far=P_FAR):
    for a in range(3):
        e = _prolong_axis(e, shape[a], a, T, near, far)
    return e


def prolong_parent(e, shape):
    return np.repeat(np.repeat(np.repeat(e, 2, 0), 2, 1), 2, 2)[:shape[0], :shape[1], :shape[2]]


# ---- the two cycles ------------------------------------------------------------------------------------------------------------
class Rediscretised:
    """M^-1 of the re-discretised cycle for one domain.  The keyword arguments exist for the mutation tests only."""

    def __init__(self, typ0, cnt0, scale, T, wc=None, elem=None, post=(MG_W2, MG_W1), near=P_NEAR, far=P_FAR, sweeps=MG_CSWEEPS,
                 coarse_colours=((0, 1), (1, 0))):
        self.T = T = np.dtype(T).type
        self.plan = plan(typ0.shape, elem if elem else (4 if T is np.float32 else 8))
        self.wc = list(self.plan["wc"] if wc is None else wc)
        self.post, self.near, self.far, self.sweeps, self.coarse_colours = post, near, far, sweeps, coarse_colours
        self.types = [typ0]
        for _ in self.plan["dims"][1:]:
            self.types.append(coarsen_types(self.types[-1]))
        assert [t.shape for t in self.types] == self.plan["dims"]
        self.ops = [op_level0(typ0, cnt0, scale, T)] + [op_rediscretised(t, scale, l, T) for l, t in enumerate(self.types) if l > 0]

    def __call__(self, b):
        T, ops = self.T, self.ops
        nl = len(ops)
        f = [np.where(ops[0].mask, b, 0).astype(T)]
        u = []
        for l in range(nl - 1):
            u.append(_pre(ops[l], f[l], MG_W1, MG_W2, T))
            r = _residual(ops[l], u[l], f[l])
            f.append(np.where(ops[l + 1].mask, restrict_trilinear(r, T, self.near, self.far), 0).astype(T))
        u.append(_rbgs(ops[-1], f[-1], self.sweeps, self.coarse_colours))
        for l in range(nl - 2, -1, -1):
            e = prolong_trilinear(u[l + 1], ops[l].mask.shape, T, self.near, self.far)
            v = np.where(ops[l].mask, u[l] + T(self.wc[l]) * e, 0).astype(T)
            for w in self.post:
                v = _sweep(ops[l], v, f[l], w, T)
            u[l] = v
        return u[0]


class Galerkin:
    """M^-1 of the cycle with Galerkin coarse levels by aggregation."""

    def __init__(self, typ0, cnt0, scale, T, inner_factor=2, w2=GAL_W2, wc=GAL_WC, sweeps=GAL_SWEEPS, lc=None, stored_rows=False):
        # lc: the coarsest level, for domains so small that the solver would not take this cycle (the reference's own tests)
        self.T = T = np.dtype(T).type
        self.plan = plan(typ0.shape, 4)
        self.lc = self.plan["gal_lc"] if lc is None else lc
        assert self.lc is not None, "no Galerkin cycle for this domain"
        self.w2, self.wc, self.sweeps = w2, wc, sweeps
        self.ops = [op_level0(typ0, cnt0, scale, T)]
        for l in range(self.lc):
            # stored_rows: the rows as the solver stores them (op_galerkin_stored) instead of the exact triple product
            self.ops.append(op_galerkin_stored(self.ops[-1], np.float32(scale) if l == 0 else None) if stored_rows
                            else op_galerkin(self.ops[-1], inner_factor))

    def __call__(self, b):
        T, ops, lc = self.T, self.ops, self.lc
        f = [np.where(ops[0].mask, b, 0).astype(T)]
        u = []
        for l in range(lc):
            w2 = MG_W2 if l == 0 else self.w2
            u.append(_pre(ops[l], f[l], GAL_W1, w2, T))
            f.append(sum8(_residual(ops[l], u[l], f[l])))
        u.append(_rbgs(ops[lc], f[lc], self.sweeps))
        for l in range(lc - 1, -1, -1):
            w2 = MG_W2 if l == 0 else self.w2
            v = np.where(ops[l].mask, u[l] + T(self.wc) * prolong_parent(u[l + 1], ops[l].mask.shape), 0).astype(T)
            v = _sweep(ops[l], v, f[l], w2, T)
            u[l] = _sweep(ops[l], v, f[l], GAL_W1, T)
        return u[0]


# ---- scenes: the container inside the default solid shell (two cells thick) ----------------------------------------------------
def shell(n):
    s = np.ones((n, n, n), dtype=np.uint8)
    s[2:n - 2, 2:n - 2, 2:n - 2] = 0
    return s


def scene(name, n, seed=0):
    """(solid, container) of the scenes of tests/test_gpu_vcycle.py at grid size n (y is up).
      tank        every non-solid cell holds water
      holes       80 % random fill and a solid block of about n / 7 cells per side in the water
      pool        water n / 10 cells deep, 40 blobs of 3^3 cells above it and a one-cell sheet
      floor       water in the lowest 3 cell layers (y < 5) over the whole floor
      floor_odd   the same, moved one cell in x and z (the cells next to the -x and -z walls stay dry)"""
    rng = np.random.default_rng(seed + 17 * n)
    solid = shell(n)
    cont = np.zeros((n, n, n), dtype=np.float32)
    inside = solid == 0
    if name == "tank":
        cont[inside] = 1
    elif name == "holes":
        k = max(2, round(n * 6 / 40))
        c = n // 2 - k // 2 + 1
        solid[c:c + k, c:c + k, c:c + k] = 1
        cont[(solid == 0) & (rng.random((n, n, n)) < 0.8)] = 1
    elif name == "pool":
        depth = max(2, round(n * 6 / 64))
        cont[:, 2:2 + depth, :] = 1
        for _ in range(40 if n >= 48 else 6):
            c = rng.integers(3, n - 6, size=3)
            c[1] = rng.integers(2 + depth + 2, n - 6)
            cont[c[0]:c[0] + 3, c[1]:c[1] + 3, c[2]:c[2] + 3] = 1
        cont[n // 4:3 * n // 4, n // 2, n // 4:3 * n // 4] = 1
        cont[~inside] = 0
    elif name in ("floor", "floor_odd"):
        o = 1 if name == "floor_odd" else 0
        cont[2 + o:, 2:5, 2 + o:] = 1
        cont[~inside] = 0
    else:
        raise ValueError(name)
    return solid, cont
