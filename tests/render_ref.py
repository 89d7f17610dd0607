"""Reference for the liquid surface as an image (include/fluid_hip.h, "liquid surface as an image") — test infrastructure, numpy only.

The definition restated on a dense val (n, n, n) float32 (tests/sdf_ref.py closed(), optionally through sdf_filter_ref.smooth):
vectorised over the pixels and over chunks of consecutive k, every sample of every ray evaluated — no skipping of any kind.  float32 wherever the
definition says float; numpy's float32 +, -, *, / and sqrt are the IEEE operations, and every product is formed before its sum.
  camera()    a Camera-like record from plain lists (what the tests hand to the library as fluid_camera_t)
  pinhole()   the pinhole of the tests, built with float64 numpy and narrowed once (NOT fluid_camera_look_at: the reference must not
              depend on the code under test)
  render()    {"rgb" (H, W, 3) uint8, "depth" (H, W) float32, "normals" (H, W, 3) float32, "n_hit", "k_hit" (H, W) int, -1: miss}
"""
from collections import namedtuple

import numpy as np

from sdf_ref import geometry

F = np.float32
Cam = namedtuple("Cam", "eye dir00 du dv width height t_near step n_steps")


def camera(eye, dir00, du, dv, width, height, t_near, step, n_steps):
    f3 = lambda v: tuple(float(F(x)) for x in v)   # noqa: E731
    return Cam(f3(eye), f3(dir00), f3(du), f3(dv), int(width), int(height), float(F(t_near)), float(F(step)), int(n_steps))


def pinhole(eye, target, up, fov_y_degrees, width, height, step, n_steps):
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    fw = target - eye
    fw /= np.linalg.norm(fw)
    rt = np.cross(fw, up)
    rt /= np.linalg.norm(rt)
    dn = np.cross(fw, rt)
    px = 2.0 * np.tan(np.radians(fov_y_degrees) / 2.0) / height
    return camera(eye, fw - 0.5 * width * px * rt - 0.5 * height * px * dn, px * rt, px * dn, width, height, 0.0, step, n_steps)


def _in_bounds(p, lo, hi):
    b0, b1 = F(lo - 1), F(hi + 1)
    with np.errstate(invalid="ignore"):
        return ((p >= b0) & (p < b1)).all(axis=-1)


def _cell(p, ok):
    """(c int64 (m, 3), f float32 (m, 3)) of the in-bounds points; c = 0, f = 0 elsewhere (callers mask)."""
    q = np.where(ok[:, None], p, F(0))
    c = np.floor(q).astype(np.int64)
    f = (q - c.astype(F)).astype(F)
    return c, f


def _corners(V, c, lo):
    """(m, 8) float32, corner dx * 4 + dy * 2 + dz; V is val padded by one voxel of +bg on every side."""
    i = c - (lo - 1)
    out = np.empty((len(c), 8), F)
    for d in range(8):
        out[:, d] = V[i[:, 0] + (d >> 2), i[:, 1] + ((d >> 1) & 1), i[:, 2] + (d & 1)]
    return out


def _lerp(a, b, t):
    d = (b - a).astype(F)
    td = (t * d).astype(F)
    return (a + td).astype(F)


def _trilinear(v, f):
    z = [_lerp(v[:, 2 * k], v[:, 2 * k + 1], f[:, 2]) for k in range(4)]
    y = [_lerp(z[0], z[1], f[:, 1]), _lerp(z[2], z[3], f[:, 1])]
    return _lerp(y[0], y[1], f[:, 0])


def value(V, p, lo, hi, bg):
    ok = _in_bounds(p, lo, hi)
    c, f = _cell(p, ok)
    c = np.where(ok[:, None], c, lo - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = _trilinear(_corners(V, c, lo), f)
    return np.where(ok, v, F(bg)).astype(F)


def _normal(v, f):
    e = (F(1) - f).astype(F)
    stride = (4, 2, 1)
    g = []
    for a in range(3):
        b1, b2 = [x for x in range(3) if x != a]
        s = np.zeros(len(v), F)
        for d1, d2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            w = ((f[:, b1] if d1 else e[:, b1]) * (f[:, b2] if d2 else e[:, b2])).astype(F)
            i0 = d1 * stride[b1] + d2 * stride[b2]
            dv = (v[:, i0 + stride[a]] - v[:, i0]).astype(F)
            s = (s + (w * dv).astype(F)).astype(F)
        g.append(s)
    l2 = (g[0] * g[0]).astype(F)
    l2 = (l2 + (g[1] * g[1]).astype(F)).astype(F)
    l2 = (l2 + (g[2] * g[2]).astype(F)).astype(F)
    ln = np.sqrt(l2).astype(F)
    some = ln > F(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.where(some, (ga / ln).astype(F), F(0)) for ga in g], axis=1).astype(F)


def _points(eye, d, t):
    """p_a = eye_a + t * d_a for t (m,) and d (m, 3)."""
    with np.errstate(invalid="ignore", over="ignore"):
        td = (np.asarray(t, dtype=F)[:, None] * d).astype(F)
        return (eye[None, :] + td).astype(F)


def render(val, bg, cam, base=(1.0, 1.0, 1.0), background=(0, 0, 0)):
    val = np.ascontiguousarray(val, dtype=F)
    n = val.shape[0]
    lo, hi, _, _ = geometry(n)
    bg = F(bg)
    V = np.full((n + 2,) * 3, bg, F)
    V[1:-1, 1:-1, 1:-1] = val
    W, H = cam.width, cam.height
    eye, dir00, du, dv = (np.array(v, dtype=F) for v in (cam.eye, cam.dir00, cam.du, cam.dv))
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pi = (ii.ravel().astype(F) + F(0.5)).astype(F)
    pj = (jj.ravel().astype(F) + F(0.5)).astype(F)
    D = ((dir00[None, :] + (pi[:, None] * du[None, :]).astype(F)).astype(F) + (pj[:, None] * dv[None, :]).astype(F)).astype(F)
    l2 = (D[:, 0] * D[:, 0]).astype(F)
    l2 = (l2 + (D[:, 1] * D[:, 1]).astype(F)).astype(F)
    l2 = (l2 + (D[:, 2] * D[:, 2]).astype(F)).astype(F)
    ln = np.sqrt(l2).astype(F)
    alive = (ln > F(0)) & np.isfinite(ln)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(alive[:, None], (D / ln[:, None]).astype(F), F(0)).astype(F)
    m = W * H
    t_near, step = F(cam.t_near), F(cam.step)
    k_hit = np.full(m, -1, np.int64)
    depth = np.full(m, np.inf, F)
    v_prev = np.zeros(m, F)                                      # value(p_{k-1}) at the first k of a chunk
    todo = alive.copy()
    K = max(1, min(cam.n_steps, 65536 // m))                     # samples per ray and chunk: every one of them is evaluated
    for k0 in range(0, cam.n_steps, K):
        if not todo.any():
            break
        ks = np.arange(k0, min(k0 + K, cam.n_steps))
        with np.errstate(over="ignore", invalid="ignore"):
            tk = (t_near + (ks.astype(F) * step).astype(F)).astype(F)
            td = (tk[None, :, None] * d[:, None, :]).astype(F)
            p = (eye[None, None, :] + td).astype(F)
        v = value(V, p.reshape(-1, 3), lo, hi, bg).reshape(m, len(ks))
        neg = v < F(0)
        first = np.where(neg.any(axis=1), neg.argmax(axis=1), -1)
        new = np.flatnonzero(todo & (first >= 0))
        if len(new):
            j = first[new]
            k = ks[j]
            v1 = v[new, j]
            v0 = np.where(j > 0, v[new, np.maximum(j - 1, 0)], v_prev[new])
            t1 = tk[j]
            with np.errstate(over="ignore", invalid="ignore"):
                t0 = (t_near + (np.maximum(k - 1, 0).astype(F) * step).astype(F)).astype(F)
                num = ((t1 - t0).astype(F) * v0).astype(F)
                den = (v0 - v1).astype(F)
                depth[new] = np.where(k == 0, t1, (t0 + (num / den).astype(F)).astype(F))
            k_hit[new] = k
            todo[new] = False
        v_prev = v[:, -1]
    hit = k_hit >= 0
    normals = np.zeros((m, 3), F)
    if hit.any():
        ph = _points(eye, d[hit], depth[hit])
        ok = _in_bounds(ph, lo, hi)
        c, f = _cell(ph, ok)
        c = np.where(ok[:, None], c, lo - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            nr = _normal(_corners(V, c, lo), f)
        normals[hit] = np.where(ok[:, None], nr, F(0))
    rgb = np.empty((m, 3), np.uint8)
    rgb[:] = np.array(background, np.uint8)
    s = (normals[:, 0] * d[:, 0]).astype(F)
    s = (s + (normals[:, 1] * d[:, 1]).astype(F)).astype(F)
    s = (s + (normals[:, 2] * d[:, 2]).astype(F)).astype(F)
    s = np.abs(s)
    for c in range(3):
        x = (F(base[c]) * s).astype(F)
        with np.errstate(invalid="ignore"):
            x = np.where(x > F(0), np.where(x < F(1), x, F(1)), F(0)).astype(F)
        b = ((x * F(255)).astype(F) + F(0.5)).astype(F).astype(np.uint8)
        rgb[hit, c] = b[hit]
    return {"rgb": rgb.reshape(H, W, 3), "depth": depth.reshape(H, W), "normals": normals.reshape(H, W, 3), "n_hit": int(hit.sum()),
            "k_hit": k_hit.reshape(H, W)}
