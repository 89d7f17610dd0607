"""The pressure matrix of setA (fluid.cc:304-412, oracle/fluid_oracle.cpp setA) restated matrix-free over the unknowns, and the
TRUE residual b - A p of a solve evaluated in extended precision.

Not a conftest: tests import it.  A solve is judged by backward errors, which do not depend on how settled the pool is:

  eta   = ||b - A p||_2 / || |A||p| + |b| ||_2            (normwise)
  omega = max_i |b - A p|_i / (|A||p| + |b|)_i           (componentwise: one wrong cell shows)

The matrix: per unknown, the diagonal is `scale` = dt / (rho dx^2) accumulated in float32 once per non-solid neighbour (cells
outside W are solid, so every neighbour of an unknown is inside the grid), the coupling to an unknown neighbour is
float32(-scale); a neighbour that is air contributes to the diagonal only (p = 0 there).  All coefficients are float32 values,
b is float32 (FLUID_FIELD_DIVER), p is float64 (FLUID_FIELD_PRESSURE): the residual is formed from exact products (Dekker's
TwoProduct) summed with TwoSum in long double, so r carries ~64 correct bits even where b and A p cancel to 1e-16.
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "the residual needs an 80-bit (or wider) long double"

LD = np.longdouble
# Dekker's splitter for a 64-bit significand: 2^32 + 1
_SPLIT = LD(2) ** 32 + 1

# Bars on the backward errors of a converged fp64 solve.  Calibration (tests/test_pressure_system.py, printed there): the
# oracle's Jacobi CG and the vendored Eigen IC-PCG reach eta 1.5e-16 ... 2.8e-16 and omega 7.4e-16 ... 4.9e-15 on the five
# awkward shapes, an obstacle scene and a 40^3 pool 30 steps in; both bars sit >= 4x above the worst of those.  omega is only
# as sharp as the rows are large: where |A||p| + |b| falls to 1e-4 of its peak (the corners of a cube in its first steps) a
# converged CG's residual is as large in absolute terms as elsewhere, and the oracle's own CG reaches omega ~1e-13 there
# (tests/test_gpu_residual.py then holds the GPU to the oracle on the same system).
ETA_BAR = 2e-15
OMEGA_BAR = 3e-14

# direction order of the neighbour columns: x-, x+, y-, y+, z-, z+
_DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def diag_table(scale):
    """diag[k] = scale added k times in float32 to 0.0f (the double sum rounded after every step, as setA does)."""
    acc, t = np.float32(0), [np.float32(0)]
    for _ in range(6):
        acc = np.float32(np.float64(acc) + np.float64(scale))
        t.append(acc)
    return np.array(t, dtype=np.float64)


class System:
    """Rows = unknowns in index order (INDICES value).  cells[i]: flat (x, y, z) cell of row i; nb[i, d]: row of the
    neighbour in direction d, -1 if it is not an unknown; count[i]: non-solid neighbours; diag[i], off: the float32 entries."""

    def __init__(self, n, cells, nb, count, diag, off, scale):
        self.n, self.cells, self.nb, self.count, self.diag, self.off, self.scale = n, cells, nb, count, diag, off, scale

    @property
    def size(self):
        return len(self.cells)

    @property
    def in_system(self):
        """Rows with a non-zero diagonal: setA2 assembles only these (an unknown walled in on all six sides has none)."""
        return self.count > 0

    def triplets(self):
        """(rows, cols, vals) of the rows in the system, sorted by (row, col): the form of oracle.system()."""
        m = self.size
        rows = [np.arange(m)]
        cols = [np.arange(m)]
        vals = [self.diag]
        for d in range(6):
            j = self.nb[:, d]
            k = j >= 0
            rows.append(np.nonzero(k)[0])
            cols.append(j[k])
            vals.append(np.full(int(k.sum()), self.off))
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        keep = self.in_system[rows]
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
        o = np.lexsort((cols, rows))
        return rows[o], cols[o], vals[o]

    def gather(self, field):
        """Values of an (n, n, n) field at the unknowns, in row order (float64)."""
        return np.asarray(field).reshape(-1)[self.cells].astype(np.float64)


def restate(solid, container_or_flags, indices, dt, rho=1.0, dx=1.0):
    """The matrix of setA for these cells.  `container_or_flags`: the CONTAINER field (fluid where > 0) or the FLAGS bytes
    (bit 1 = fluid); only used to check that the unknowns are exactly the fluid cells.  Gathers the unknowns and their six
    neighbours: cost proportional to the unknowns, not to N^3."""
    solid = np.asarray(solid).reshape(-1)
    idx = np.asarray(indices).reshape(-1)
    n = round(len(idx) ** (1.0 / 3.0))
    assert n ** 3 == len(idx)
    flat = np.flatnonzero(idx >= 0)
    m = len(flat)
    rows = idx[flat].astype(np.int64)
    assert np.array_equal(np.sort(rows), np.arange(m)), "INDICES is not a numbering 0..m-1"
    cells = np.empty(m, dtype=np.int64)
    cells[rows] = flat
    cof = np.asarray(container_or_flags).reshape(-1)
    fluid = (cof & 2) != 0 if cof.dtype == np.uint8 else cof > 0
    assert np.array_equal(fluid & (solid == 0), idx >= 0), "the unknowns are not the non-solid fluid cells"
    x, r = np.divmod(cells, n * n)
    y, z = np.divmod(r, n)
    assert x.min(initial=1) > 0 and x.max(initial=0) < n - 1 and y.min(initial=1) > 0 and y.max(initial=0) < n - 1 \
        and z.min(initial=1) > 0 and z.max(initial=0) < n - 1, "an unknown on the grid's outer layer"
    scale = np.float64(dt) / (np.float64(rho) * np.float64(dx) * np.float64(dx))
    nb = np.empty((m, 6), dtype=np.int64)
    count = np.zeros(m, dtype=np.int64)
    for d, (ax, ay, az) in enumerate(_DIRS):
        c = cells + (ax * n + ay) * n + az
        count += solid[c] == 0
        nb[:, d] = idx[c]
    nb[nb < 0] = -1
    diag = diag_table(scale)[count]
    off = np.float64(np.float32(-scale))
    return System(n, cells, nb, count, diag, off, scale)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _measures(r, mag, b):
    r = np.asarray(r, dtype=LD)
    mag = np.asarray(mag, dtype=LD)
    b = np.asarray(b, dtype=LD)
    nr = np.sqrt(np.sum(r * r))
    nm = np.sqrt(np.sum(mag * mag))
    nb = np.sqrt(np.sum(b * b))
    ar = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(mag > 0, ar / np.where(mag > 0, mag, 1), np.where(ar > 0, np.inf, 0))
    return {"eta": float(nr / nm) if nm > 0 else 0.0, "omega": float(q.max(initial=0)),
            "relres": float(nr / nb) if nb > 0 else float(nr), "worst_row": int(np.argmax(q)) if len(q) else -1,
            "rnorm": float(nr), "bnorm": float(nb)}


def residual(sys, b, p, rows=None):
    """r = b - A p, |A||p| + |b| and the backward errors, over the rows of the system (or the subset `rows`).
    b, p: per-row float64 arrays (p of every unknown: a row's neighbours may lie outside `rows`).
    Returns a dict: r, mag (long double arrays over the rows checked), rows, eta, omega, relres, worst_row (a row id)."""
    if rows is None:
        rows = np.nonzero(sys.in_system)[0]
    rows = np.asarray(rows, dtype=np.int64)
    bl = np.asarray(b, dtype=np.float64)[rows].astype(LD)
    pl = np.asarray(p, dtype=np.float64).astype(LD)
    diag = sys.diag[rows].astype(LD)
    off = LD(sys.off)
    # terms: b, -diag p_i, -off p_j for every unknown neighbour j (exact products, compensated sum)
    s, c = bl, np.zeros_like(bl)
    ph, pl_ = _two_prod(-diag, pl[rows])
    s, e = _two_sum(s, ph)
    c = c + e + pl_
    mag = np.abs(bl) + np.abs(diag * pl[rows])
    for d in range(6):
        j = sys.nb[rows, d]
        pj = np.where(j >= 0, pl[np.maximum(j, 0)], LD(0))
        ph, pl_ = _two_prod(-off, pj)
        s, e = _two_sum(s, ph)
        c = c + e + pl_
        mag = mag + np.abs(off * pj)
    r = s + c
    out = _measures(r, mag, bl)
    out["worst_row"] = int(rows[out["worst_row"]]) if out["worst_row"] >= 0 else -1
    out.update(r=r, mag=mag, rows=rows)
    return out


def components(sys, b, p, comp_cells):
    """The measures of residual() restricted to each cell list of comp_cells (e.g. the droplets of fluid_get_droplets: an array of
    flat cell indices per component, padded with -1).  Returns one dict per component (eta, omega, relres, rows)."""
    row_of = np.full(sys.n ** 3, -1, dtype=np.int64)
    row_of[sys.cells] = np.arange(sys.size)
    out = []
    for cells in comp_cells:
        cells = np.asarray(cells, dtype=np.int64)
        cells = cells[cells >= 0]
        rows = row_of[cells]
        assert (rows >= 0).all(), "a component cell that is not an unknown"
        res = residual(sys, b, p, rows)
        out.append({k: res[k] for k in ("eta", "omega", "relres", "rows", "worst_row")})
    return out


def check_field_solve(solid, flags, indices, diver, pressure, dt, rho=1.0, dx=1.0):
    """restate + residual straight from the simulation's fields (FLAGS, INDICES, DIVER, PRESSURE and the step's dt):
    also checks that the restated counts are the FLAGS count bits and that p = 0 off the unknowns.  Returns (sys, residual dict)."""
    flags = np.asarray(flags)
    sys = restate(solid, flags, indices, dt, rho, dx)
    fl = flags.reshape(-1)[sys.cells]
    assert np.array_equal(((fl >> 2) & 7).astype(np.int64), sys.count), "FLAGS count bits differ from the restated neighbour counts"
    pr = np.asarray(pressure).reshape(-1)
    off = np.ones(pr.size, dtype=bool)
    off[sys.cells[sys.in_system]] = False
    assert not pr[off].any(), "non-zero pressure outside the system's unknowns"
    return sys, residual(sys, sys.gather(diver), sys.gather(pressure))
