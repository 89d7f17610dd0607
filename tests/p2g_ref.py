"""The exact per-cell sums of particle -> grid, and the bars a float implementation of them may be held to.

Not a conftest: tests import it.  Restated from the reference (fluid.cc:265-299 p2gCatmullRom, 843-882 interpolate, 1106-1148
P2Gtransfer) and include/fluid_hip.h, never from the kernels.

A cell receives an addend from a particle iff it is one of the 27 cells around round(pos) (C round), lies inside
W = [2, n-3] on every axis and is not solid.  The addend's weight is the reference's double product cw = (sx * sy) * sz of
three spline values: a deterministic double, the same wherever it is evaluated.  Everything after that is exact here:

  k      number of addends with cw != 0                (cw == 0 adds exactly nothing anywhere)
  Wp     sum cw                                        what P2Gtransfer's `weights` approximates (no sign test, :288-293)
  Wc     sum of the cw > 0                             what interpolate's `container` approximates (cw > 0, :870)
  N[a]   sum cw * v_a  (the product exact as well)     the numerator of the velocity
  T[a]   sum |cw * v_a|,  A = sum |cw|                 the scales of the bars

Wp, Wc and N are returned as double-double pairs (X, X_lo): X is the exact sum correctly rounded to double, X + X_lo agrees
with it to ~2^-100 of the sum of magnitudes.  How: the addends of a cell are scaled by a power of two so that the largest is
below 1, cut into four slices of 26 bits and a tail, and each slice is summed as integers held in doubles (exact below 2^53,
i.e. for fewer than 2^25 addends per cell and call); products are split into (p, e) with p + e = cw * v exactly (Dekker).
T and A are sums of non-negative terms in np.longdouble: a few units of 2^-53 relative, they only scale bars.

The spline goes negative: for 1 - 6.5e-6 < |x| < 1 the written expression returns rounding noise of either sign around
2 (1 - |x|)^3 < 5e-16.  Such "grazing" addends count in k, Wp, N, T, A; Wc leaves the negative ones out, like the reference.
"""
import numpy as np

from sources_ref import c_round, spline

U24 = 2.0 ** -24
U53 = 2.0 ** -53
_SPLIT = 134217729.0  # 2^27 + 1
_NSLICE = 4


# ---- error-free pieces --------------------------------------------------------------------------------------------------
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def two_prod(a, b):
    """p + e == a * b exactly (Dekker / Veltkamp; no overflow or underflow at the magnitudes of a particle step)."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ahi, alo, bhi, blo):
    s, e = two_sum(ahi, bhi)
    e = e + (alo + blo)
    return fast_two_sum(s, e)


def seg_exact(arrs, starts, counts):
    """Per segment, the exact sum of all the arrays' entries as a double-double (hi, lo)."""
    m = np.zeros(len(starts))
    for a in arrs:
        m = np.maximum(m, np.maximum.reduceat(np.abs(a), starts))
    _, e = np.frexp(m)                     # m < 2^e (e = 0 where m == 0)
    er = np.repeat(e, counts)
    ys = [np.ldexp(a, -er) for a in arrs]  # |y| < 1, exact
    terms = []
    for j in range(_NSLICE):
        tot = np.zeros(len(starts))
        for i, y in enumerate(ys):
            t = y * 67108864.0             # 2^26, exact
            c = np.rint(t)
            ys[i] = t - c                  # exact, |.| <= 1/2
            tot += np.add.reduceat(c, starts)   # integers below 2^53: exact in any order
        terms.append(np.ldexp(tot, -26 * (j + 1)))
    tail = np.zeros(len(starts))
    for y in ys:
        tail += np.add.reduceat(y, starts)
    terms.append(np.ldexp(tail, -26 * _NSLICE))
    hi = np.zeros(len(starts))
    lo = np.zeros(len(starts))
    for t in terms:
        hi, lo = dd_add(hi, lo, t, 0.0)
    return np.ldexp(hi, e), np.ldexp(lo, e)


# ---- the addends ---------------------------------------------------------------------------------------------------------
def addends(pos, vel, n, solid=None, planes=None, round_fn=c_round, w_margin=2, assoc="xy_z"):
    """Every (particle, cell) pair with cw != 0 as flat arrays: (particle index, linear cell, cw).  round_fn, w_margin and
    assoc exist for the mutation tests only (another rounding rule, a wider W, sx * (sy * sz))."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    glo = -(n // 2)
    lo, hi = float(w_margin), float(n - 1 - w_margin)
    base = round_fn(pos) - glo                       # index space, float (a far-away particle stays a float)
    pid = np.arange(len(pos))
    if planes is not None:
        pl = np.asarray(sorted(planes), dtype=np.float64)
        near = np.zeros(len(pos), dtype=bool)
        for p in pl:
            near |= np.abs(base[:, 0] - p) <= 1
        pid = pid[near]
    ok = np.all((base[pid] >= lo - 1) & (base[pid] <= hi + 1), axis=1)   # some neighbour inside W
    pid = pid[ok]
    b = base[pid].astype(np.int64)
    p = pos[pid]
    s = np.empty((3, 3, len(pid)))                   # axis, offset, particle
    for a in range(3):
        for d in range(3):
            s[a, d] = spline(p[:, a] - (b[:, a] + (d - 1) + glo).astype(np.float64))
    out_p, out_c, out_w = [], [], []
    sol = None if solid is None else np.asarray(solid).reshape(-1) != 0
    for dx in range(3):
        x = b[:, 0] + dx - 1
        okx = (x >= lo) & (x <= hi)
        if planes is not None:
            okx &= np.isin(x, np.asarray(list(planes), dtype=np.int64))
        for dy in range(3):
            y = b[:, 1] + dy - 1
            okxy = okx & (y >= lo) & (y <= hi)
            for dz in range(3):
                z = b[:, 2] + dz - 1
                if assoc == "xy_z":
                    cw = (s[0, dx] * s[1, dy]) * s[2, dz]
                else:
                    cw = s[0, dx] * (s[1, dy] * s[2, dz])
                keep = okxy & (z >= lo) & (z <= hi) & (cw != 0)
                lin = (x[keep] * n + y[keep]) * n + z[keep]
                cwk = cw[keep]
                pk = pid[keep]
                if sol is not None:
                    open_ = ~sol[lin]
                    lin, cwk, pk = lin[open_], cwk[open_], pk[open_]
                out_p.append(pk); out_c.append(lin); out_w.append(cwk)
    if not out_p:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(out_p), np.concatenate(out_c), np.concatenate(out_w)


class P2GRef:
    """The exact sums over the cells that receive something (ascending linear index in `cell`)."""

    def __init__(self, n):
        self.n = n
        self.cell = np.zeros(0, np.int64)
        self.k = np.zeros(0, np.int64)
        self.kneg = np.zeros(0, np.int64)            # addends with cw < 0
        self.Wp, self.Wp_lo, self.Wc, self.Wc_lo = (np.zeros(0) for _ in range(4))
        self.N, self.N_lo, self.T = (np.zeros((3, 0)) for _ in range(3))
        self.A = np.zeros(0)
        self.cwmax = np.zeros(0)                     # the largest single addend

    def _merge(self, o):
        """Add the sums of another chunk of particles (double-double additions: 2^-104 relative each)."""
        cell = np.union1d(self.cell, o.cell)
        ia, ib = np.searchsorted(cell, self.cell), np.searchsorted(cell, o.cell)
        r = P2GRef(self.n)
        r.cell = cell
        m = len(cell)

        def put(a, b, dtype=np.float64, shape=(), fill=0):
            x = np.full(shape + (m,), fill, dtype=dtype); y = np.full(shape + (m,), fill, dtype=dtype)
            x[..., ia] = a; y[..., ib] = b
            return x, y
        for name in ("k", "kneg"):
            x, y = put(getattr(self, name), getattr(o, name), np.int64)
            setattr(r, name, x + y)
        for name in ("Wp", "Wc"):
            ah, bh = put(getattr(self, name), getattr(o, name))
            al, bl = put(getattr(self, name + "_lo"), getattr(o, name + "_lo"))
            h, l = dd_add(ah, al, bh, bl)
            setattr(r, name, h); setattr(r, name + "_lo", l)
        ah, bh = put(self.N, o.N, shape=(3,))
        al, bl = put(self.N_lo, o.N_lo, shape=(3,))
        r.N, r.N_lo = dd_add(ah, al, bh, bl)
        x, y = put(self.T, o.T, np.longdouble, (3,)); r.T = x + y
        x, y = put(self.A, o.A, np.longdouble); r.A = x + y
        x, y = put(self.cwmax, o.cwmax, fill=-np.inf); r.cwmax = np.maximum(x, y)
        return r

    # ---- what the reference's fields must look like -------------------------------------------------------------------
    def dense(self, name):
        """A per-cell array (n^3, zeros where nothing arrives) of `k`, `A`, `Wp`, `Wc`."""
        a = getattr(self, name)
        d = np.zeros(self.n ** 3, dtype=a.dtype)
        d[self.cell] = a
        return d

    def sign_split(self):
        """Linear indices of the cells whose P2G weight and container sums differ in sign (grazing addends only)."""
        return self.cell[np.sign(self.Wp) != np.sign(self.Wc)]

    def flag_split(self):
        """... and of those where it shows in the fluid flag: the reference marks a cell fluid where container > 0 (Wc > 0); one
        array serving as both container and weights marks it where Wp > 0."""
        return self.cell[(self.Wc > 0) != (self.Wp > 0)]


def _chunk_ref(pos, vel, n, idx, **kw):
    pid, lin, cw = addends(pos[idx], vel[idx], n, **kw)
    r = P2GRef(n)
    if len(lin) == 0:
        return r
    o = np.argsort(lin, kind="stable")
    lin, cw, pid = lin[o], cw[o], pid[o]
    cell, starts, counts = np.unique(lin, return_index=True, return_counts=True)
    r.cell, r.k = cell, counts.astype(np.int64)
    r.kneg = np.add.reduceat((cw < 0).astype(np.int64), starts)
    r.Wp, r.Wp_lo = seg_exact([cw], starts, counts)
    r.Wc, r.Wc_lo = seg_exact([np.where(cw > 0, cw, 0.0)], starts, counts)
    r.A = np.add.reduceat(np.abs(cw).astype(np.longdouble), starts)
    r.cwmax = np.maximum.reduceat(cw, starts)
    v = vel[idx][pid]
    N, Nl, T = [], [], []
    for a in range(3):
        p, e = two_prod(cw, v[:, a])
        h, l = seg_exact([p, e], starts, counts)
        N.append(h); Nl.append(l)
        T.append(np.add.reduceat(np.abs(p).astype(np.longdouble), starts))
    r.N, r.N_lo, r.T = np.array(N), np.array(Nl), np.array(T)
    return r


def p2g_ref(pos, vel, n, solid=None, planes=None, chunk=100000, **kw):
    """The exact sums for particles (pos, vel) on an n^3 grid.  solid: optional (n, n, n) mask of cells that receive nothing
    (the shell outside W needs no entry: W is tested by itself).  planes: restrict the result to these x indices (index
    space); only the particles whose base x is within one cell of one of them are looked at."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    vel = np.zeros_like(pos) if vel is None else np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    r = P2GRef(n)
    for i0 in range(0, len(pos), chunk):
        c = _chunk_ref(pos, vel, n, np.arange(i0, min(i0 + chunk, len(pos))), solid=solid, planes=planes, **kw)
        if len(c.cell):
            r = c if len(r.cell) == 0 else r._merge(c)
    return r


def cell_addends(pos, vel, n, cell, **kw):
    """The addends of one cell, for a failing cell's post-mortem: (particle index, cw), in particle order."""
    pid, lin, cw = addends(pos, vel, n, **kw)
    m = lin == cell
    o = np.argsort(pid[m], kind="stable")
    return pid[m][o], cw[m][o]


# ---- the bars ------------------------------------------------------------------------------------------------------------
def gamma(k, u):
    k = np.asarray(k, dtype=np.longdouble)
    return k * u / (1 - k * u)


class Verdict:
    """Per-cell ratios of error to bar, and the cells that break one."""

    def __init__(self):
        self.bad = []        # (what, linear cell, value, bar)
        self.ratio = {}      # what -> largest error / bar

    def cells(self, what=None):
        return sorted({c for w, c, _, _ in self.bad if what is None or w == what})

    def __bool__(self):
        return not self.bad

    def describe(self, n, limit=6):
        out = []
        for w, c, v, b in self.bad[:limit]:
            out.append(f"{w}: cell {c} = ({c // (n * n)}, {c // n % n}, {c % n}) error {float(v):.3e} bar {float(b):.3e}")
        return f"{len(self.bad)} violations; " + "; ".join(out)


def check_fields(ref, weights, vel, container=None, solid=None, narrowings=None, grazing=False, planes=None):
    """Hold float fields (weights (n,n,n) float32, vel (3,n,n,n) float64, as P2Gtransfer leaves them) to the exact sums.

    weight bar       |w - Wp| <= gamma(k, 2^-24) A                        k float32 narrowings in any order
    numerator bar    |u_a double(w) - N_a| <= gamma(k + 4, 2^-53) T_a     where w > 0; where w <= 0 the reference does not
                     divide and u_a itself is the numerator.  One product rounding and <= k - 1 additions in any order, two
                     more roundings for another association of the product, the division and the product undoing it.
    support          w > 0 exactly where one addend alone is visible in float32 (float32(cw) > 0); w == 0 where A < 2^-150;
                     `ambiguous` counts the cells in between (callers assert 0).  Outside the support (and in solid cells)
                     every field is exactly 0.  grazing=True: cells with a negative addend are left out of the sign rule.
    project bar      narrowings=m: |w - Wp| <= (m 2^-24 + (k + 2) 2^-53) A  (double partials, narrowed m times), first order.
    container        if given: equals weights bit for bit (grazing=False).
    planes           restrict "exactly 0 elsewhere" to these x planes (a reference computed for some planes only).
    """
    n = ref.n
    v = Verdict()
    w = np.asarray(weights).reshape(-1)
    u = np.asarray(vel).reshape(3, -1)
    LD = np.longdouble
    c = ref.cell
    wc = w[c].astype(np.float64)
    k = ref.k

    def hold(what, err, bar, cells):
        err = np.asarray(err, dtype=LD); bar = np.asarray(bar, dtype=LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))
        v.ratio[what] = max(v.ratio.get(what, 0.0), float(r.max()) if r.size else 0.0)
        for i in np.nonzero(err > bar)[0]:
            v.bad.append((what, int(cells[i]), err[i], bar[i]))

    # weight, reference bar
    ew = np.abs(LD(1) * wc - (LD(1) * ref.Wp + ref.Wp_lo))
    hold("weight", ew, gamma(k, U24) * ref.A, c)
    if narrowings is not None:
        hold("weight_project", ew, (narrowings * U24 + (k + 2) * U53) * ref.A, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        v.ratio["weight_over_u24A"] = float(np.max(np.where(ref.A > 0, ew / (U24 * ref.A), 0))) if len(c) else 0.0
    # numerator
    div = np.where(wc > 0, wc, 1.0)
    for a in range(3):
        num = LD(1) * u[a][c] * div
        hold("numerator", np.abs(num - (LD(1) * ref.N[a] + ref.N_lo[a])), gamma(k + 4, U53) * ref.T[a], c)
    # support
    seen = np.float32(ref.cwmax) > 0
    none = ref.A < 2.0 ** -150
    rule = np.ones(len(c), dtype=bool) if not grazing else ref.kneg == 0
    v.ambiguous = int(np.sum(rule & ~seen & ~none))
    for i in np.nonzero(rule & seen & ~(wc > 0))[0]:
        v.bad.append(("support", int(c[i]), wc[i], 0.0))
    for i in np.nonzero(rule & none & (wc != 0))[0]:
        v.bad.append(("support", int(c[i]), wc[i], 0.0))
    # exactly nothing elsewhere
    outside = np.ones(n ** 3, dtype=bool)
    outside[c] = False
    if planes is not None:
        inpl = np.zeros((n, n * n), dtype=bool)
        inpl[np.asarray(list(planes), dtype=np.int64)] = True
        outside &= inpl.reshape(-1)
    stale = outside & ((w != 0) | (u[0] != 0) | (u[1] != 0) | (u[2] != 0))
    if container is not None:
        stale |= outside & (np.asarray(container).reshape(-1) != 0)
    for i in np.nonzero(stale)[0]:
        v.bad.append(("outside_support", int(i), w[i], 0.0))
    if solid is not None:
        s = np.asarray(solid).reshape(-1) != 0
        for i in np.nonzero(s & ((w != 0) | (u[0] != 0) | (u[1] != 0) | (u[2] != 0)))[0]:
            v.bad.append(("solid", int(i), w[i], 0.0))
    if container is not None and not grazing:
        cb = np.asarray(container).reshape(-1)
        for i in np.nonzero(cb.view(np.uint32) != w.view(np.uint32))[0]:
            if planes is None or (i // (n * n)) in set(planes):
                v.bad.append(("container_is_weights", int(i), cb[i], w[i]))
    return v
