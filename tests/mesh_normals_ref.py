"""Reference for the mesh's normals and triangles (include/fluid_hip.h, "liquid surface as a mesh: normals and triangles") — test
infrastructure, numpy only, written from the definition.  float32 wherever the definition says float; numpy's float32 add, subtract,
multiply, divide and sqrt are the IEEE operations, and a product is rounded before it is added (no FMA).
  offsets(val)      f (3, m, m, m) float32 = s_axis / (float)k per cell (NaN where the cell is not mixed), and the mixed mask:
                    s and k recomputed as tests/mesh_ref.py's mesh() forms them, f is NOT vertex - c
  normals(val)      (nv, 3) float32 in mesh_ref.mesh(val)'s vertex order
  cell_normal(c, f) the same for one cell, scalar by scalar: c (2, 2, 2) corner values indexed [dx, dy, dz], f the three offsets;
                    `swap` and `pairs` give the wrong forms the order test compares against
  triangles(v, q)   (2 nq, 3) uint32
"""
import numpy as np

import mesh_ref
from sdf_ref import geometry

F = np.float32
PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1))


def offsets(val):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    m = n - 1

    def corner(d):
        return val[d[0]:d[0] + m, d[1]:d[1] + m, d[2]:d[2] + m]
    inside = np.zeros((m, m, m), int)
    for d in np.ndindex(2, 2, 2):
        inside += corner(d) < F(0)
    mixed = (inside > 0) & (inside < 8)
    s = np.zeros((3, m, m, m), F)
    k = np.zeros((m, m, m), int)
    zero = F(0)
    for a in range(3):
        b1, b2 = [x for x in range(3) if x != a]
        for d1, d2 in PAIRS:
            d0 = [0, 0, 0]
            d0[b1], d0[b2] = d1, d2
            e = list(d0)
            e[a] = 1
            v0, v1 = corner(d0), corner(e)
            counts = (v0 < zero) != (v1 < zero)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = v0 / (v0 - v1)
            s[a] = s[a] + np.where(counts, t, zero)
            s[b1] = s[b1] + np.where(counts, F(d1), zero)
            s[b2] = s[b2] + np.where(counts, F(d2), zero)
            k += counts
    with np.errstate(divide="ignore", invalid="ignore"):
        f = s / k.astype(F)
    assert f.dtype == F
    return f, mixed, corner


def normals(val):
    """(normals (nv, 3) float32, len (nv,) float32 — the gradient's length before the division) in the mesh's vertex order."""
    f, mixed, corner = offsets(val)
    n = np.asarray(val).shape[0]
    lo = geometry(n)[0]
    one = F(1)
    e = one - f
    g = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            b1, b2 = [x for x in range(3) if x != a]
            ga = np.zeros(mixed.shape, F)
            for d1, d2 in PAIRS:
                d0 = [0, 0, 0]
                d0[b1], d0[b2] = d1, d2
                d1c = list(d0)
                d1c[a] = 1
                w1 = f[b1] if d1 else e[b1]
                w2 = f[b2] if d2 else e[b2]
                ga = ga + (w1 * w2) * (corner(d1c) - corner(d0))
            assert ga.dtype == F
            g.append(ga)
        l2 = g[0] * g[0]
        l2 = l2 + g[1] * g[1]
        l2 = l2 + g[2] * g[2]
        ln = np.sqrt(l2)
        assert ln.dtype == F
    ci = np.argwhere(mixed)
    ci = ci[mesh_ref._order(ci + lo)]
    ix = (ci[:, 0], ci[:, 1], ci[:, 2])
    lv = ln[ix]
    some = lv > F(0)                                             # False for a NaN too
    out = np.zeros((len(ci), 3), F)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            out[:, a] = np.where(some, g[a][ix] / lv, F(0))
    return out, lv


def cell_normal(c, f, swap=False, pairs=PAIRS):
    """One cell, scalar float32 operations in the stated order.  swap: b1 and b2 exchanged (a wrong form); pairs: another
    summation order (a wrong form).  Returns (normal (3,) float32, len)."""
    c = np.asarray(c, dtype=F)
    f = [F(x) for x in f]
    g = []
    for a in range(3):
        b1, b2 = [x for x in range(3) if x != a]
        if swap:
            b1, b2 = b2, b1
        ga = F(0)
        for d1, d2 in pairs:
            i0 = [0, 0, 0]
            i0[b1], i0[b2] = d1, d2
            i1 = list(i0)
            i1[a] = 1
            w1 = f[b1] if d1 else F(1) - f[b1]
            w2 = f[b2] if d2 else F(1) - f[b2]
            w = F(w1 * w2)
            dv = F(c[tuple(i1)] - c[tuple(i0)])
            ga = F(ga + F(w * dv))
        g.append(ga)
    l2 = F(g[0] * g[0])
    l2 = F(l2 + F(g[1] * g[1]))
    l2 = F(l2 + F(g[2] * g[2]))
    ln = F(np.sqrt(l2))
    if not ln > F(0):
        return np.zeros(3, F), ln
    return np.array([F(x / ln) for x in g], F), ln


def cell_offsets(c):
    """f of one mixed cell, c (2, 2, 2): the mesh definition's s_axis / (float)k, scalar by scalar."""
    c = np.asarray(c, dtype=F)
    s = [F(0), F(0), F(0)]
    k = 0
    for a in range(3):
        b1, b2 = [x for x in range(3) if x != a]
        for d1, d2 in PAIRS:
            i0 = [0, 0, 0]
            i0[b1], i0[b2] = d1, d2
            i1 = list(i0)
            i1[a] = 1
            v0, v1 = c[tuple(i0)], c[tuple(i1)]
            if (v0 < 0) == (v1 < 0):
                continue
            s[a] = F(s[a] + F(v0 / F(v0 - v1)))
            s[b1] = F(s[b1] + F(d1))
            s[b2] = F(s[b2] + F(d2))
            k += 1
    return [F(x / F(k)) for x in s]


def diagonals(vertices, quads):
    """(d02, d13) float32 per quad: dx*dx, then + dy*dy, then + dz*dz over float differences."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i, j in ((0, 2), (1, 3)):
            d = v[q[:, j]] - v[q[:, i]]
            s = d[:, 0] * d[:, 0]
            s = s + d[:, 1] * d[:, 1]
            s = s + d[:, 2] * d[:, 2]
            assert s.dtype == F
            out.append(s)
    return out


def triangles(vertices, quads):
    """(2 nq, 3) uint32, and cut13 (nq,) bool: which quads were cut along b-d."""
    q = np.asarray(quads, dtype=np.uint32).reshape(-1, 4)
    d02, d13 = diagonals(vertices, q)
    cut13 = d13 < d02                                            # False for ties and NaN
    a, b, c, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    t0 = np.stack([a, b, np.where(cut13, d, c)], axis=1)
    t1 = np.stack([np.where(cut13, b, a), c, d], axis=1)
    return np.stack([t0, t1], axis=1).reshape(-1, 3).astype(np.uint32), cut13


# ---- per scene, computed once per process, never modified -------------------------------------------------------------------------
_cache = {}


def scene(name, n, R, w, dx, filt=None):
    """(val, (vertices, quads, cells), normals, len, triangles) of a scene of tests/mesh_ref.py, val filtered by filt; cached."""
    import sdf_filter_ref
    import sdf_ref
    key = (name, n, R, w, dx, filt)
    if key not in _cache:
        _, val, act, m = mesh_ref.scene(name, n, R, w, dx)
        if filt is not None:
            val = sdf_filter_ref.smooth(val, act, sdf_ref.constants(R, w, dx)[3], *filt)
            m = mesh_ref.mesh(val)
        nr, ln = normals(val)
        tri, _ = triangles(m[0], m[1])
        for a in (nr, ln, tri):
            a.setflags(write=False)
        _cache[key] = (val, m[:3], nr, ln, tri)
    return _cache[key]
