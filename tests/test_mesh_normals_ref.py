"""CPU (-m "not gpu"): the numpy reference of the mesh's normals and triangles (tests/mesh_normals_ref.py) against the properties the
definition promises — unit length, orientation out of the liquid, triangles that keep their quads' entries, winding and volume — and
the term order pinned on an asymmetric hand-made cell.  The hand-made cases are also what the host functions give
(fluid_sdf_mesh_normals, fluid_mesh_triangles), bit for bit."""
import numpy as np
import pytest

import mesh_normals_ref as mn
import mesh_ref
import sdf_ref
from sdf_testlib import u32

SETS = mesh_ref.SETS
N = 32


@pytest.fixture(autouse=True)
def _the_feature_is_built(fs):
    """Every test here is about an entry point this library must have."""
    assert fs.lib.fluid_sdf_mesh_normals and fs.lib.fluid_mesh_triangles


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner", "lo", "hi", "cloud"])
def test_unit_length(name, R, w, dx):
    """| |n|^2 - 1 | <= 1e-6 in double wherever len > 0: three correctly rounded divisions, the rounded length (a square root of a
    sum of three rounded squares): about 7 roundings of 2^-24 on |n|^2, 4.2e-7."""
    _, (vert, _, _), nr, ln, _ = mn.scene(name, N, R, w, dx)
    assert len(nr) == len(vert) > 0 and nr.dtype == np.float32
    some = ln > 0
    err = np.abs((nr[some].astype(np.float64) ** 2).sum(axis=1) - 1.0)
    assert err.max() <= 1e-6, (name, err.max())
    assert (u32(nr[~some]) == 0).all()                                           # +0.0f, all three
    assert np.isfinite(nr).all()


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner"])
def test_normals_point_away_from_the_particle(name, R, w, dx):
    _, (vert, _, _), nr, ln, _ = mn.scene(name, N, R, w, dx)
    pos = mesh_ref.positions(name, N)[0]
    r = vert.astype(np.float64) - pos
    r /= np.linalg.norm(r, axis=1)[:, None]
    dots = (nr.astype(np.float64) * r).sum(axis=1)
    assert (ln > 0).all() and dots.min() > 0, (name, dots.min())


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner", "lo", "hi"])
def test_normals_agree_with_the_quads_winding(name, R, w, dx):
    """n . (geometric quad normal) > 0 at all four corners of every non-degenerate quad.  (The cloud gets no such assertion: its
    under-resolved sheets have opposed normals, a property of surface nets on thin features.)"""
    _, (vert, quads, _), nr, _, _ = mn.scene(name, N, R, w, dx)
    v = vert.astype(np.float64)
    q = quads.astype(np.int64)
    qn = np.cross(v[q[:, 2]] - v[q[:, 0]], v[q[:, 3]] - v[q[:, 1]])             # counter-clockwise seen from outside: outward
    area = np.linalg.norm(qn, axis=1)
    ok = area > 1e-9
    assert ok.sum() > 0
    qn = qn[ok] / area[ok, None]
    for k in range(4):
        dots = (nr[q[ok, k]].astype(np.float64) * qn).sum(axis=1)
        assert dots.min() > 0, (name, k, dots.min())


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner", "lo", "hi", "cloud"])
def test_triangles_keep_their_quads(name, R, w, dx):
    _, (vert, quads, _), _, _, tri = mn.scene(name, N, R, w, dx)
    tri2, cut13 = mn.triangles(vert, quads)
    assert np.array_equal(tri, tri2) and tri.dtype == np.uint32 and tri.shape == (2 * len(quads), 3)
    pair = tri.reshape(-1, 2, 3).astype(np.int64)
    q = quads.astype(np.int64)
    for i in range(len(q)):
        t0, t1 = pair[i]
        assert set(t0) | set(t1) == set(q[i]), i                                 # exactly the quad's entries
        dia = {q[i, 1], q[i, 3]} if cut13[i] else {q[i, 0], q[i, 2]}
        assert dia <= set(t0) and dia <= set(t1), i                              # both hold the chosen diagonal
    # the quad's winding: each triangle is a cyclic sub-sequence of (a, b, c, d)
    a, b, c, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    exp0 = np.where(cut13[:, None], np.stack([a, b, d], 1), np.stack([a, b, c], 1))
    exp1 = np.where(cut13[:, None], np.stack([b, c, d], 1), np.stack([a, c, d], 1))
    assert np.array_equal(pair[:, 0], exp0) and np.array_equal(pair[:, 1], exp1)
    if name == "cloud":
        assert 0 < cut13.sum() < len(q)                                          # both branches are taken


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner", "cloud"])
def test_signed_volume_is_positive_under_either_cut(name, R, w, dx):
    _, (vert, quads, _), _, _, tri = mn.scene(name, N, R, w, dx)
    assert mesh_ref.is_closed(quads)
    v02 = mesh_ref.signed_volume(vert, quads)                                    # (a, b, c), (a, c, d)
    v13 = mesh_ref.signed_volume(vert, np.roll(quads, -1, axis=1))               # (b, c, d), (b, d, a)
    mine = mesh_ref.signed_volume(vert, np.concatenate([tri, tri[:, 2:]], axis=1))   # (t0, t1, t2) and a null triangle
    assert v02 > 0 and v13 > 0 and mine > 0, (v02, v13, mine)


def test_hand_made_quads_take_the_stated_branch(fs):
    nan = np.float32(np.nan)
    v = np.array([[0, 0, 0], [1, 0, 0], [3, 3, 0], [0, 1, 0],                    # quad 0: d02 = 18, d13 = 2   -> cut b-d
                  [0, 0, 1], [3, 0, 1], [1, 1, 1], [0, 3, 1],                    # quad 1: d02 = 2,  d13 = 18  -> cut a-c
                  [0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2],                    # quad 2: a tie                 -> cut a-c
                  [0, 0, 3], [nan, 0, 3], [9, 9, 3], [0, 1, 3],                  # quad 3: d13 is NaN            -> cut a-c
                  [0, 0, 4], [1, 0, 4], [nan, 9, 4], [0, 1, 4]], np.float32)     # quad 4: d02 is NaN            -> cut a-c
    q = np.arange(20, dtype=np.uint32).reshape(5, 4)
    d02, d13 = mn.diagonals(v, q)
    assert (d02[0], d13[0], d02[1], d13[1], d02[2], d13[2]) == (18, 2, 2, 18, 2, 2) and np.isnan(d13[3]) and np.isnan(d02[4])
    tri, cut13 = mn.triangles(v, q)
    assert cut13.tolist() == [True, False, False, False, False]
    assert tri[:2].tolist() == [[0, 1, 3], [1, 2, 3]]
    for i in range(1, 5):
        a = 4 * i
        assert tri[2 * i:2 * i + 2].tolist() == [[a, a + 1, a + 2], [a, a + 2, a + 3]], i
    assert np.array_equal(fs.mesh_triangles(v, q), tri)
    # degenerate quads are kept: all four entries the same vertex
    deg = np.array([[5, 5, 5, 5]], np.uint32)
    assert mn.triangles(v, deg)[0].tolist() == [[5, 5, 5], [5, 5, 5]] and np.array_equal(fs.mesh_triangles(v, deg), mn.triangles(v, deg)[0])


CELL = np.array([[[-0.3, 0.7], [0.45, 1.1]], [[0.2, -0.9], [1.3, 0.05]]], np.float32)   # [dx, dy, dz]: no symmetry on any axis


def test_term_order_is_pinned_by_an_asymmetric_cell(fs):
    """b1 < b2 and the (0,0), (0,1), (1,0), (1,1) order: exchanging the two other axes or reversing the sum changes the bits of
    this cell's normal, and the dense form and the host function give the stated form's bits."""
    f = mn.cell_offsets(CELL)
    right, ln = mn.cell_normal(CELL, f)
    assert ln > 0
    swapped, _ = mn.cell_normal(CELL, f, swap=True)
    backwards, _ = mn.cell_normal(CELL, f, pairs=mn.PAIRS[::-1])
    assert not np.array_equal(u32(right), u32(swapped)) and not np.array_equal(u32(right), u32(backwards))
    assert np.allclose(right, swapped, atol=1e-6) and np.allclose(right, backwards, atol=1e-6)   # the same vector, other roundings
    # the cell in a grid of its own: min corner (0, 0, 0) of a 16^3 grid, everything else +bg ... which makes neighbours mixed too
    n, bg = 16, np.float32(2.0)
    lo = sdf_ref.geometry(n)[0]
    val = np.full((n, n, n), bg, np.float32)
    val[-lo:-lo + 2, -lo:-lo + 2, -lo:-lo + 2] = CELL
    vert, _, cells, _ = mesh_ref.mesh(val)
    nr, _ = mn.normals(val)
    k = int(np.flatnonzero((cells == 0).all(axis=1))[0])
    assert np.array_equal(u32(nr[k]), u32(right))
    # f is s / k, not vertex - c: for this cell at this place the two agree or not, the definition does not care; at a far cell
    # the add rounds and they differ (tests/test_mesh_normals_host.py covers whole scenes)
    act = val != bg
    org, lv, la = sdf_ref.leaf_list(val, act, bg)
    got = fs.sdf_mesh_normals(fs.SdfGrid(n, org, lv, la, bg, 3.0, 1.0))
    assert np.array_equal(u32(got), u32(nr))


def test_offsets_are_s_over_k_not_vertex_minus_cell():
    """Somewhere in the cloud (float)c + f rounds, so vertex - c is not f: the reference takes f before the add."""
    val, (vert, _, cells), nr, _, _ = mn.scene("cloud", N, *SETS[0])
    f, mixed, _ = mn.offsets(val)
    lo = sdf_ref.geometry(N)[0]
    ci = cells - lo
    fv = np.stack([f[a][ci[:, 0], ci[:, 1], ci[:, 2]] for a in range(3)], axis=1)
    assert np.array_equal(u32(cells.astype(np.float32) + fv), u32(vert))
    assert (u32(vert - cells.astype(np.float32)) != u32(fv)).any()
