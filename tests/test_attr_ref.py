"""CPU (-m "not gpu"): tests/attr_ref.py against itself — the closed form of the closest particle equals the particle-by-particle
loop in both visiting orders, exact ties go to the smaller id whatever the order, and the filtered scenes really do have
counting edges with a single active end (a condition on the inputs the host and GPU tests rely on)."""
import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_ref
from sdf_testlib import u32

SETS = mesh_ref.SETS
NO_ID = attr_ref.NO_ID


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("name", ["one", "corner", "lo", "hi", "cloud"])
def test_closed_form_is_the_sequential_loop_in_both_orders(name, R, w, dx):
    n = 25
    pos, vel, _, act, ids, v32 = attr_ref.scene(name, n, R, w, dx)[:6]
    assert act.any() and (ids[act] < len(pos)).all() and (ids[~act] == NO_ID).all()
    assert (u32(v32)[:, ~act] == 0).all()                                        # +0.0f, not -0.0f
    assert np.array_equal(u32(v32[:, act]), u32(vel.astype(np.float32)[ids[act]].T))
    for order in (None, range(len(pos) - 1, -1, -1)):
        i2, v2 = attr_ref.sequential(pos, vel, n, R, w, dx, order)
        assert np.array_equal(i2, ids) and np.array_equal(u32(v2), u32(v32))
    if name == "cloud":                                                          # a voxel's winner really is (one of) the nearest
        P, _ = sdf_ref.counted(pos, n)
        assert len(P) == len(pos) and len(np.unique(ids[act])) > 100


def test_tie_plane_goes_to_the_smaller_id_in_both_upload_orders():
    n, (R, w, dx) = 16, SETS[0]
    pos, vel = attr_ref.tie_scene()
    lo = sdf_ref.geometry(n)[0]
    for p, v in ((pos, vel), (pos[::-1], vel[::-1])):
        ids, v32 = attr_ref.closest(p, v, n, R, w, dx)
        _, act = sdf_ref.closed(p, n, R, w, dx)
        x = np.arange(n) + lo
        plane = act[x == 0][0]
        assert plane.sum() > 20
        d0 = sdf_ref.dist2(0, *np.meshgrid(x, x, indexing="ij"), p[0])
        d1 = sdf_ref.dist2(0, *np.meshgrid(x, x, indexing="ij"), p[1])
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))           # exact ties, every voxel of the plane
        assert (ids[x == 0][0][plane] == 0).all()                               # row 0 wins either way
        assert np.array_equal(u32(v32[:, x == 0][:, 0][:, plane]), u32(np.repeat(v[0].astype(np.float32)[:, None], plane.sum(), 1)))
        near = 0 if p[0, 0] < 0 else 1                                           # off the plane: the nearer particle
        assert (ids[x < 0][act[x < 0]] == near).all() and (ids[x > 0][act[x > 0]] == 1 - near).all()
        for order in (None, (1, 0)):
            i2, v2 = attr_ref.sequential(p, v, n, R, w, dx, order)
            assert np.array_equal(i2, ids) and np.array_equal(u32(v2), u32(v32))


@pytest.mark.parametrize("name,n,filt,two,one,nv", [
    ("cloud", 25, None, 13016, 0, 3243),
    ("cloud", 25, (4, 3, 0.0), 6876, 2916, 2448),
    ("cloud", 25, (1, 0, -0.9), 2656, 11760, 3593),
    ("dilate5", 32, (1, 0, -0.9), 0, 1248, 314),
])
def test_edge_classes_of_the_shared_scenes(name, n, filt, two, one, nv):
    """Where the one-ended rule is exercised: never without a filter, always with one at (R, w) = (3, 1); no edge without an
    active end anywhere."""
    R, w, dx = 3.0, 1.0, 1.0
    if name == "dilate5":
        pos = np.array([[-4.49, -4.49, -4.49]])
        val, act = sdf_ref.closed(pos, n, R, w, dx)
        import sdf_filter_ref
        val = sdf_filter_ref.smooth(val, act, sdf_ref.constants(R, w, dx)[3], *filt)
        _, v32 = attr_ref.closest(pos, np.array([[1.0, -2.0, 0.5]]), n, R, w, dx)
        vv, classes = attr_ref.vertex_velocity(val, act, v32)
        assert np.array_equal(u32(vv), u32(np.tile(np.float32([1.0, -2.0, 0.5]), (nv, 1))))
    else:
        sc = attr_ref.scene(name, n, R, w, dx, filt)
        vv, classes = sc[6]
        assert len(sc[7][0]) == nv                                               # mesh_ref's vertices: the same cells, the same order
    assert classes == {"two": two, "one": one, "none": 0, "vertices": nv, "empty": 0, "partial": 0}
    assert vv.shape == (nv, 3) and np.isfinite(vv).all()


def test_vertex_velocity_of_a_uniform_field_is_that_field():
    """Every contributing edge gives a0 + t * 0 = a0, so the mean is the field up to the rounding of the sum / count."""
    n, (R, w, dx) = 16, SETS[0]
    pos = mesh_ref.positions("one", n)
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    _, v32 = attr_ref.closest(pos, np.array([[0.5, -2.0, 4.0]]), n, R, w, dx)   # (exact in float, and so are their small multiples)
    vv, classes = attr_ref.vertex_velocity(val, act, v32)
    assert classes["one"] == 0 and classes["none"] == 0 and classes["two"] > 0
    assert np.allclose(vv, [0.5, -2.0, 4.0], rtol=1e-6, atol=0)
