"""Reference for the liquid surface as a mesh (include/fluid_hip.h, "liquid surface as a mesh") — test infrastructure, numpy only.

Naive surface nets on the voxel grid, written from the definition: from a dense val (n, n, n) float32 (tests/sdf_ref.py closed()),
one vertex per cell whose eight corners disagree in sign, one quad per grid edge whose two ends disagree in sign and whose four
cells exist.  float32 wherever the definition says float; numpy's float32 add, subtract and divide are the IEEE operations.
  mesh()      (vertices (nv, 3) float32, quads (nq, 4) uint32, cells (nv, 3) int — the min corner of each vertex's cell,
              t — every edge parameter that was used)
  and the checks the tests share: directed / undirected edge counts, closedness, Euler characteristic, signed volume.
"""
import numpy as np

from sdf_ref import geometry

F = np.float32


def _order(c, extra=None):
    """Permutation that sorts the voxels c (k, 3) by leaf origin (x, y, z), then offset ((x&7)*8 + (y&7))*8 + (z&7), then extra."""
    org = c & ~7
    off = ((c[:, 0] & 7) * 8 + (c[:, 1] & 7)) * 8 + (c[:, 2] & 7)
    keys = [off, org[:, 2], org[:, 1], org[:, 0]]
    if extra is not None:
        keys.insert(0, extra)
    return np.lexsort(keys)


def mesh(val):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    lo, hi, _, _ = geometry(n)
    m = n - 1                                                    # cells per axis: c in [lo, hi - 1]
    inside = val < F(0)

    def corner(a, d):                                            # a[c + d] for every cell c
        return a[d[0]:d[0] + m, d[1]:d[1] + m, d[2]:d[2] + m]
    cnt = np.zeros((m, m, m), int)
    for d in np.ndindex(2, 2, 2):
        cnt += corner(inside, d)
    mixed = (cnt > 0) & (cnt < 8)
    s = np.zeros((3, m, m, m), F)
    k = np.zeros((m, m, m), int)
    ts = []
    for a in range(3):
        b1, b2 = [x for x in range(3) if x != a]                 # the two other axes, ascending
        for d1, d2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            d0 = [0, 0, 0]
            d0[b1], d0[b2] = d1, d2
            e = list(d0)
            e[a] = 1
            v0, v1 = corner(val, d0), corner(val, e)
            counts = (v0 < F(0)) != (v1 < F(0))
            with np.errstate(divide="ignore", invalid="ignore"):
                t = v0 / (v0 - v1)
            assert t.dtype == F
            ts.append(t[counts])
            zero = F(0)
            s[a] = s[a] + np.where(counts, t, zero)
            s[b1] = s[b1] + np.where(counts, F(d1), zero)
            s[b2] = s[b2] + np.where(counts, F(d2), zero)
            k += counts
    assert ((k > 0) == mixed).all()
    ci = np.argwhere(mixed)                                      # array indices of the mixed cells
    c = ci + lo
    p = _order(c)
    ci, c = ci[p], c[p]
    kk = k[ci[:, 0], ci[:, 1], ci[:, 2]].astype(F)
    vert = np.stack([c[:, x].astype(F) + s[x][ci[:, 0], ci[:, 1], ci[:, 2]] / kk for x in range(3)], axis=1).astype(F)
    num = np.full((m, m, m), -1, np.int64)
    num[ci[:, 0], ci[:, 1], ci[:, 2]] = np.arange(len(ci))

    P, A = [], []
    for a in range(3):
        b, cc = (a + 1) % 3, (a + 2) % 3
        e = [0, 0, 0]
        e[a] = 1
        # p_a in [lo, hi - 1], p_b and p_c in [lo + 1, hi - 1], as array indices
        sl = [None] * 3
        sl[a], sl[b], sl[cc] = slice(0, n - 1), slice(1, n - 1), slice(1, n - 1)
        sl1 = list(sl)
        sl1[a] = slice(1, n)
        diff = inside[tuple(sl)] != inside[tuple(sl1)]
        pi = np.argwhere(diff)
        pi[:, b] += 1
        pi[:, cc] += 1
        P.append(pi)
        A.append(np.full(len(pi), a))
    P, A = np.concatenate(P), np.concatenate(A)
    o = _order(P + lo, A)
    P, A = P[o], A[o]
    quads = np.empty((len(P), 4), np.int64)
    for i, (pi, a) in enumerate(zip(P, A)):
        b, cc = (a + 1) % 3, (a + 2) % 3
        eb, ec = np.zeros(3, int), np.zeros(3, int)
        eb[b], ec[cc] = 1, 1
        q = [num[tuple(pi - eb - ec)], num[tuple(pi - ec)], num[tuple(pi)], num[tuple(pi - eb)]]
        quads[i] = q if inside[tuple(pi)] else [q[0], q[3], q[2], q[1]]
    assert (quads >= 0).all()                                    # all four cells are mixed by construction
    return vert, quads.astype(np.uint32), c, (np.concatenate(ts) if ts else np.empty(0, F))


def directed_edges(quads):
    """{(i, j): how many quads run i -> j}; degenerate edges (i == i) are left out."""
    q = np.asarray(quads, dtype=np.int64)
    out = {}
    for k in range(4):
        for i, j in zip(q[:, k].tolist(), q[:, (k + 1) % 4].tolist()):
            if i != j:
                out[(i, j)] = out.get((i, j), 0) + 1
    return out


def is_closed(quads):
    """Every directed edge i -> j is matched by as many j -> i."""
    d = directed_edges(quads)
    return len(d) > 0 and all(d.get((j, i), 0) == c for (i, j), c in d.items())


def undirected_uses(quads):
    """{frozen edge: number of quads that use it}."""
    out = {}
    for (i, j), c in directed_edges(quads).items():
        key = (min(i, j), max(i, j))
        out[key] = out.get(key, 0) + c
    return out


def euler(vertices, quads):
    return len(vertices) - len(undirected_uses(quads)) + len(quads)


def signed_volume(vertices, quads):
    """Divergence theorem over the quads split into the triangles (0, 1, 2) and (0, 2, 3), in double."""
    v = np.asarray(vertices, dtype=np.float64)
    q = np.asarray(quads, dtype=np.int64)
    vol = 0.0
    for tri in ((0, 1, 2), (0, 2, 3)):
        a, b, c = v[q[:, tri[0]]], v[q[:, tri[1]]], v[q[:, tri[2]]]
        vol += np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    return vol


# ---- the scenes the mesh tests share: computed once per process, never modified -------------------------------------------------
SETS = [(1.5, 2.5, 1.0), (3.0, 1.0, 1.0), (1.0, 2.0, 0.5), (2.0, 2.0, 1.0)]      # (R, w, dx), those of tests/test_gpu_sdf.py


def positions(name, n):
    lo, hi, _, _ = geometry(n)
    if name == "one":
        return np.array([[0.3, -0.2, 0.41]])
    if name == "corner":                                         # eight leaves meet at (-0.5, -0.5, -0.5)
        return np.array([[-0.5, -0.5, -0.5]])
    if name == "lo":                                             # cut by the grid's lo face: an open mesh
        return np.array([[lo + 0.4, 0.0, 0.0]])
    if name == "hi":
        return np.array([[0.2, hi - 0.3, hi - 1.1], [hi - 0.1, hi - 0.2, -2.6]])
    if name == "cloud":
        return np.random.default_rng(300).uniform(-8.0, 8.0, (300, 3))
    raise KeyError(name)


_cache = {}


def scene(name, n, R, w, dx):
    """(positions, val, act, (vertices, quads, cells, t)) of a named scene; cached."""
    import sdf_ref
    key = (name, n, R, w, dx)
    if key not in _cache:
        pos = positions(name, n)
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        for a in (pos, val, act):
            a.setflags(write=False)
        _cache[key] = (pos, val, act, mesh(val))
    return _cache[key]
