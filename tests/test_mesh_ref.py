"""CPU (-m "not gpu"): the definition of the liquid surface as a mesh (include/fluid_hip.h, "liquid surface as a mesh") as
tests/mesh_ref.py states it, on tests/sdf_ref.py closed() grids: a sphere away from the grid faces is a closed, outward-oriented
quad mesh of Euler characteristic 2; a sphere the grid face cuts is open there; a cloud is closed with non-manifold dual edges;
every vertex lies in its own cell and every edge parameter in (0, 1]."""
import numpy as np
import pytest

import mesh_ref
import sdf_ref

SETS = mesh_ref.SETS


def in_own_cell(vert, cells, t):
    d = vert.astype(np.float64) - cells
    assert ((d >= 0.0) & (d <= 1.0)).all()
    assert ((t > 0) & (t <= 1)).all() and t.dtype == np.float32


@pytest.mark.parametrize("R,w,dx", SETS)
def test_one_sphere_is_closed_and_oriented(R, w, dx):
    n = 16
    lo, hi, _, _ = sdf_ref.geometry(n)
    _, val, _, (vert, quads, cells, t) = mesh_ref.scene("one", n, R, w, dx)
    assert len(vert) > 0 and len(quads) > 0
    assert (cells > lo).all() and (cells < hi - 1).all()                       # away from the grid faces
    assert mesh_ref.is_closed(quads)
    assert mesh_ref.euler(vert, quads) == 2
    vol = mesh_ref.signed_volume(vert, quads)
    assert vol > 0
    in_own_cell(vert, cells, t)


def test_sphere_cut_by_the_grid_face_is_open():
    n, (R, w, dx) = 16, (3.0, 1.0, 1.0)
    lo, hi, _, _ = sdf_ref.geometry(n)
    _, val, _, (vert, quads, cells, t) = mesh_ref.scene("lo", n, R, w, dx)
    assert (val[0] < 0).any()                                                   # the liquid reaches the outermost voxel layer
    assert len(quads) > 0 and not mesh_ref.is_closed(quads)
    qc = cells[quads.astype(np.int64)]                                          # (nq, 4, 3): the cells the quads refer to
    assert (qc >= lo).all() and (qc <= hi - 1).all()
    assert (cells[:, 0] == lo).any()                                            # vertices on the boundary layer of cells exist
    in_own_cell(vert, cells, t)


def test_cloud_is_closed_with_non_manifold_edges():
    n, (R, w, dx) = 25, (1.0, 1.0, 1.0)
    _, _, _, (vert, quads, cells, t) = mesh_ref.scene("cloud", n, R, w, dx)
    assert len(quads) > 1000
    assert mesh_ref.is_closed(quads)
    uses = np.array(list(mesh_ref.undirected_uses(quads).values()))
    assert (uses == 4).any() and (uses % 2 == 0).all()
    in_own_cell(vert, cells, t)


def test_order_and_counts():
    """Vertices ascend by (leaf origin, offset) of their cell, one per mixed cell; every quad joins four distinct existing cells
    that pairwise touch."""
    n, (R, w, dx) = 25, (1.0, 1.0, 1.0)
    _, val, _, (vert, quads, cells, _) = mesh_ref.scene("cloud", n, R, w, dx)
    off = ((cells[:, 0] & 7) * 8 + (cells[:, 1] & 7)) * 8 + (cells[:, 2] & 7)
    keys = [tuple(o) + (f,) for o, f in zip((cells & ~7).tolist(), off.tolist())]
    assert keys == sorted(set(keys))                                            # strictly ascending: one vertex per cell
    lo = sdf_ref.geometry(n)[0]
    inside = val < 0
    k = sum(inside[d[0]:d[0] + n - 1, d[1]:d[1] + n - 1, d[2]:d[2] + n - 1].astype(int) for d in np.ndindex(2, 2, 2))
    assert len(vert) == int(((k > 0) & (k < 8)).sum())
    qc = cells[quads.astype(np.int64)]
    assert (np.abs(qc - qc[:, :1]).max(axis=(1, 2)) <= 1).all()
    assert (np.abs(qc[:, 0] - qc[:, 2]).sum(axis=1) == 2).all()                 # Q0 and Q2 are diagonal


def test_an_all_outside_or_all_inside_grid_has_no_mesh():
    for v in (2.5, -2.5):
        vert, quads, cells, t = mesh_ref.mesh(np.full((9, 9, 9), v, np.float32))
        assert vert.shape == (0, 3) and quads.shape == (0, 4) and len(t) == 0


def test_eight_leaf_corner_scene_touches_all_neighbours():
    """The scene is what it is meant to be: quads whose four cells lie in different leaves, on every axis."""
    _, _, _, (vert, quads, cells, _) = mesh_ref.scene("corner", 16, *SETS[1])
    leaves = (cells & ~7)[quads.astype(np.int64)]                                # (nq, 4, 3)
    spread = (leaves.max(axis=1) - leaves.min(axis=1)) // 8                      # (nq, 3)
    assert {tuple(s) for s in spread.tolist()} >= {(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)}
    assert len({tuple(o) for o in (cells & ~7).tolist()}) == 8
