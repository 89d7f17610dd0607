"""GPU (-m gpu): the liquid surface's attributes (fluid_sdf_snapshot_attr / fluid_mesh_snapshot_attr and their waits; the ARGMIN
search, the attr pack and the attr emit kernels).  In every comparison the device result equals tests/attr_ref.py AND the host
functions (fluid_sdf_attr_to_dense, fluid_sdf_mesh_attr) applied to the same snapshot: ids exactly, floats as bit patterns; and the
geometry of an attribute snapshot is byte for byte the plain snapshot's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import attr_ref
import mesh_ref
import sdf_filter_ref
import sdf_ref
from sdf_testlib import u32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = mesh_ref.SETS
ERR_ARG, ERR_STATE = 1, 3
LEAF, ATTR = 2048 + 64 + 12, 2048 + 6144


def reference(pos, vel, n, R, w, dx, filt=None):
    """(val, act, ids, v32, vertex velocity, classes, (vertices, quads)) of a particle set, val filtered by filt."""
    val, act = sdf_ref.closed(pos, n, R, w, dx)
    ids, v32 = attr_ref.closest(pos, vel, n, R, w, dx)
    if filt is not None:
        val = sdf_filter_ref.smooth(val, act, sdf_ref.constants(R, w, dx)[3], *filt)
    vv, classes = attr_ref.vertex_velocity(val, act, v32)
    return val, act, ids, v32, vv, classes, mesh_ref.mesh(val)[:2]


def named(name, n, R, w, dx, filt=None):
    pos, vel, val, act, ids, v32, (vv, classes), m = attr_ref.scene(name, n, R, w, dx, filt)
    return pos, vel, (val, act, ids, v32, vv, classes, m[:2])


def same_grid(a, b, what):
    assert np.array_equal(a.origin, b.origin) and np.array_equal(u32(a.values), u32(b.values)) and np.array_equal(a.active, b.active), what
    assert (a.n, a.background.tobytes(), a.radius.tobytes(), a.half_width.tobytes()) == (b.n, b.background.tobytes(), b.radius.tobytes(), b.half_width.tobytes()), what


def check(fs, sim, ref, n, R, w, dx, filt=None, what="", plain=True):
    """Surface and mesh attribute snapshots of the handle's particles against `ref` = reference(...), against the host functions on
    the same snapshot, and (plain) their geometry against the plain snapshots of the same particles."""
    val, act, ids, v32, vv, classes, (vert, quads) = ref
    what = f"{what} {(R, w, dx)} {filt}"
    bg = sdf_ref.constants(R, w, dx)[3]
    org, lv, la = sdf_ref.leaf_list(val, act, bg)
    li, lvel = attr_ref.leaf_attr(ids, v32, org)
    sim.sdf_snapshot(R, w, smooth=filt, attr=True)
    g, at = sim.sdf_wait_attr()
    assert np.array_equal(g.origin, org) and np.array_equal(u32(g.values), u32(lv)) and np.array_equal(g.active, la), what
    assert at is not None and at.id.dtype == np.uint32 and at.velocity.dtype == np.float32
    assert np.array_equal(at.id, li), what
    assert np.array_equal(u32(at.velocity), u32(lvel)), what
    assert (at.id[~g.active] == attr_ref.NO_ID).all() and (u32(at.velocity).transpose(0, 2, 1)[~g.active] == 0).all(), what
    assert sim.sdf_stats()["bytes_to_host"] == len(org) * (LEAF + ATTR) + 4, what
    di, dv = fs.sdf_attr_to_dense(g, at)
    assert np.array_equal(di, ids) and np.array_equal(u32(dv), u32(v32)), what + " (host dense)"
    sim.mesh_snapshot(R, w, smooth=filt, attr=True)
    v, q, vel = sim.mesh_wait_attr()
    assert v.shape == vert.shape and q.shape == quads.shape, (what, v.shape, vert.shape, q.shape, quads.shape)
    assert np.array_equal(u32(v), u32(vert)) and np.array_equal(q, quads), what
    assert sim.mesh_stats() == {"vertices": len(vert), "quads": len(quads), "bytes_to_host": 24 * len(vert) + 16 * len(quads) + 8}, what
    if len(vert):
        assert vel is not None and vel.shape == vv.shape and np.array_equal(u32(vel), u32(vv)), what
        assert np.array_equal(u32(fs.sdf_mesh_attr(g, at)), u32(vel)), what + " (host mesher)"
    else:
        assert vel is None, what
    if plain:                                                                   # same geometry, and the plain waits' byte counts
        sim.sdf_snapshot(R, w, smooth=filt)
        same_grid(sim.sdf_wait(), g, what + " (plain surface)")
        assert sim.sdf_stats()["bytes_to_host"] == len(org) * LEAF + 4, what
        sim.mesh_snapshot(R, w, smooth=filt)
        pv, pq = sim.mesh_wait()
        assert np.array_equal(u32(pv), u32(v)) and np.array_equal(pq, q), what + " (plain mesh)"
        assert sim.mesh_stats()["bytes_to_host"] == 12 * len(vert) + 16 * len(quads) + 8, what
    return g, at, (v, q, vel)


@pytest.mark.parametrize("R,w,dx", SETS)
@pytest.mark.parametrize("n", [16, 25])
def test_one_particle(fs, n, R, w, dx):
    pos, vel, ref = named("one", n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    g, at, (v, q, vv) = check(fs, sim, ref, n, R, w, dx)
    assert (at.id[g.active] == 0).all() and len(v) > 0
    assert np.allclose(vv, vel[0].astype(np.float32), rtol=1e-6)                 # one particle: a uniform field
    sim.close()


@pytest.mark.parametrize("name,n,prm", [("corner", 16, SETS[0]), ("corner", 16, SETS[1]), ("lo", 16, SETS[1]), ("lo", 25, SETS[0]),
                                        ("hi", 16, SETS[1]), ("hi", 25, SETS[3])])
def test_corner_and_grid_faces(fs, name, n, prm):
    """"corner": eight leaves meet, vertex velocities read the neighbour leaves at +1; "lo" / "hi": clipped cells at the grid faces,
    two particles with different velocities in "hi"."""
    R, w, dx = prm
    pos, vel, ref = named(name, n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    g, at, _ = check(fs, sim, ref, n, R, w, dx, what=name)
    if name == "corner":
        assert g.n_leaves == 8
    if name == "hi":
        assert set(np.unique(at.id[g.active]).tolist()) == {0, 1}
    sim.close()


@pytest.mark.parametrize("flip", [False, True])
def test_tie_plane(fs, flip):
    """Two particles mirrored in x = 0: the plane's voxels are exactly tied and take row 0's velocity in either upload order."""
    n, (R, w, dx) = 16, SETS[0]
    pos, vel = attr_ref.tie_scene()
    if flip:
        pos, vel = pos[::-1].copy(), vel[::-1].copy()
    ref = reference(pos, vel, n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    g, at, _ = check(fs, sim, ref, n, R, w, dx, what=f"tie flip={flip}")
    di, dv = fs.sdf_attr_to_dense(g, at)
    _, act = fs.sdf_to_dense(g)
    x = np.arange(n) + sdf_ref.geometry(n)[0]
    plane = act[x == 0][0]
    assert plane.sum() > 20 and (di[x == 0][0][plane] == 0).all()
    assert (u32(dv[:, x == 0][:, 0][:, plane]) == u32(vel[0].astype(np.float32))[:, None]).all()
    near = 0 if pos[0, 0] < 0 else 1
    assert (di[x < 0][act[x < 0]] == near).all() and (di[x > 0][act[x > 0]] == 1 - near).all()
    sim.close()


@pytest.mark.parametrize("R,w", [(3.0, 1.0), (1.5, 2.5)])
def test_crowded_cell(fs, R, w):
    """200 particles in one cell plus the cloud (ring 4, long ranges per cell), and exact duplicates of three of them with higher
    ids and other velocities: wherever a duplicated particle is the nearest, the lower id must win."""
    n, dx = 25, 1.0
    rng = np.random.default_rng(41)
    crowd = np.array([9.0, -9.0, 9.0]) + rng.uniform(-0.5, 0.5, (200, 3))
    pos = np.concatenate([crowd, mesh_ref.positions("cloud", n)])
    ids, _ = attr_ref.closest(pos, np.zeros_like(pos), n, R, w, dx)
    dup = np.unique(ids[ids < 200])[:3]                                          # three of the crowd that own voxels
    assert len(dup) == 3
    pos = np.concatenate([pos, pos[dup]])
    vel = attr_ref.velocities(pos, seed=5)
    ref = reference(pos, vel, n, R, w, dx)
    assert (ref[2][ref[1]] < len(pos) - 3).all() and np.isin(dup, ref[2][ref[1]]).all()
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    check(fs, sim, ref, n, R, w, dx, what="crowd")
    sim.close()


def test_after_steps_the_live_order_is_not_the_id_order(fs):
    """The drop scene uploaded in a random order, 3 steps, then the download (id order) is the reference's input.  After a step the
    live arrays are in the step's cell order, so an id taken from a sorted position or from an index in the live arrays is wrong."""
    n, (R, w, dx) = 32, SETS[0]
    rng = np.random.default_rng(9)
    pos = fs.water_cube_drop(n, 4, seed=0)
    pos = pos[rng.permutation(len(pos))]
    sim = fs.FluidSim(n=n)
    sim.upload_particles(pos)
    for _ in range(3):
        sim.step()
    p, v = sim.download_particles()
    assert np.abs(v).max() > 0.1
    # id order is no cell order on any axis (the live arrays are cell-sorted by the step: were they in id order too, the base cells
    # along the sort's major axis would almost never descend from one id to the next)
    c = sdf_ref.base_cell(p)
    assert min((np.diff(c[:, a]) < 0).mean() for a in range(3)) > 0.25
    ref = reference(p, v, n, R, w, dx)
    g, at, (vert, q, vv) = check(fs, sim, ref, n, R, w, dx, what="after 3 steps")
    assert len(q) > 100 and np.abs(vv).max() > 0.1
    # ... and the ids are not the places their particles have in the snapshot's own cell order (z fastest
    # over the base-cell box, the order of the sorted scratch): a winner's place lies in its cell's range [start, start + count)
    lo_c = c.min(axis=0)
    dims = c.max(axis=0) - lo_c + 1
    key = ((c[:, 0] - lo_c[0]) * dims[1] + (c[:, 1] - lo_c[1])) * dims[2] + (c[:, 2] - lo_c[2])
    cnt = np.bincount(key, minlength=int(dims.prod()))
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    ids0 = at.id[g.active].astype(np.int64)                                      # every active voxel's winner
    assert len(ids0) > 170
    in_own_range = (ids0 >= start[key[ids0]]) & (ids0 < start[key[ids0]] + cnt[key[ids0]])
    assert in_own_range.mean() < 0.5
    sim.close()


@pytest.mark.parametrize("filt", [(4, 3, 0.0), (1, 0, -0.9)])
def test_filtered_cloud(fs, filt):
    """One-ended edges (tests/test_attr_ref.py counts them); ids and voxel velocities are the unfiltered ones."""
    n, (R, w, dx) = 25, (3.0, 1.0, 1.0)
    pos, vel, ref = named("cloud", n, R, w, dx, filt)
    assert ref[5]["one"] > 2000 and ref[5]["none"] == 0
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    g, at, _ = check(fs, sim, ref, n, R, w, dx, filt, what="cloud")
    sim.sdf_snapshot(R, w, attr=True)
    g0, at0 = sim.sdf_wait_attr()
    assert np.array_equal(g0.origin, g.origin) and np.array_equal(at0.id, at.id) and np.array_equal(u32(at0.velocity), u32(at.velocity))
    assert not np.array_equal(u32(g0.values), u32(g.values))
    sim.close()


def test_filtered_mesh_reaches_the_fifth_ring(fs):
    """One particle at (-4.49)^3, n = 32, (R, w) = (3, 1), offset -0.9: the mesh's range is the box dilated by 5, 314 vertices,
    every counting edge has one active end."""
    n, (R, w, dx), filt = 32, (3.0, 1.0, 1.0), (1, 0, -0.9)
    pos, vel = np.array([[-4.49, -4.49, -4.49]]), np.array([[1.0, -2.0, 0.5]])
    ref = reference(pos, vel, n, R, w, dx, filt)
    assert ref[5] == {"two": 0, "one": 1248, "none": 0, "vertices": 314, "empty": 0, "partial": 0}
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    _, _, (v, q, vv) = check(fs, sim, ref, n, R, w, dx, filt, what="dilate 5")
    assert len(v) == 314 and np.array_equal(u32(vv), u32(np.tile(np.float32([1.0, -2.0, 0.5]), (314, 1))))
    sim.close()


def test_cloud_and_stale_scratch(fs):
    """The cloud, then particles far from where the cloud's listed leaves were, then the cloud again, attribute snapshots only: the
    search leaves the unreached leaves of the new range at once, their ids and velocities in the scratch are the cloud's and must
    not be read."""
    n, (R, w, dx) = 25, (1.0, 1.0, 1.0)
    pos, vel, ref = named("cloud", n, R, w, dx)
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(pos, vel)
    check(fs, sim, ref, n, R, w, dx, what="cloud", plain=False)
    for p in ([[10.3, 10.2, -9.6]], [[10.3, 10.2, -9.6], [-10.4, -9.7, 10.1]]):
        far = np.array(p)
        fv = attr_ref.velocities(far, seed=3)
        sim.upload_particles(far, fv)
        r1 = reference(far, fv, n, R, w, dx)
        assert 0 < len(r1[6][0]) < 100
        check(fs, sim, r1, n, R, w, dx, what=f"particles {p} after the cloud", plain=False)
        sim.upload_particles(pos, vel)
        check(fs, sim, ref, n, R, w, dx, what="cloud again", plain=False)
    sim.close()


def test_interleaving_lifetimes_and_stats(fs):
    n, (R, w, dx) = 32, SETS[0]
    sim = fs.FluidSim(n=n)
    h = sim._h
    prm = fs.SdfParams(R, w)
    g, a, m, ma = fs.SdfGridC(), fs.SdfAttrC(), fs.MeshC(), fs.MeshAttrC()
    assert fs.lib.fluid_sdf_wait_attr(h, C.byref(g), C.byref(a)) == ERR_STATE and fs.lib.fluid_mesh_wait_attr(h, C.byref(m), C.byref(ma)) == ERR_STATE
    assert fs.lib.fluid_sdf_snapshot_attr(h, None, None) == ERR_ARG and fs.lib.fluid_mesh_snapshot_attr(h, None, None) == ERR_ARG
    assert fs.lib.fluid_sdf_snapshot_attr(h, C.byref(fs.SdfParams(2.0, 2.5)), None) == ERR_ARG
    assert fs.lib.fluid_mesh_snapshot_attr(h, C.byref(prm), C.byref(fs.SdfFilter(5, 1, 0.0))) == ERR_ARG
    # no particle at all: counts 0, NULL pointers, the header bytes alone
    sim.sdf_snapshot(R, w, attr=True)
    sim.mesh_snapshot(R, w, attr=True)
    assert fs.lib.fluid_sdf_wait_attr(h, C.byref(g), C.byref(a)) == 0 and fs.lib.fluid_mesh_wait_attr(h, C.byref(m), C.byref(ma)) == 0
    assert (g.n_leaves, g.values, a.n_leaves, a.id, a.velocity) == (0, None, 0, None, None)
    assert (m.n_vertices, m.n_quads, m.vertices, ma.n_vertices, ma.velocity) == (0, 0, None, 0, None)
    assert sim.sdf_stats()["bytes_to_host"] == 4 and sim.mesh_stats()["bytes_to_host"] == 8
    # particles, but no active voxel: outside the grid's reach (base cells off the grid are not counted)
    sim.upload_particles(np.array([[100.0, 0.0, 0.0]]), np.array([[1.0, 1.0, 1.0]]))
    sim.sdf_snapshot(R, w, attr=True)
    assert sim.sdf_wait_attr()[1] is None and sim.sdf_stats()["leaves_listed"] == 0

    p1 = fs.water_cube_drop(n, 4, seed=0)
    v1 = attr_ref.velocities(p1, seed=1)
    sim.upload_particles(p1, v1)
    sim.sdf_snapshot(R, w, attr=True)                                            # q: with attributes
    sim.mesh_snapshot(R, w, attr=True)
    sim.step()
    p2, v2 = sim.download_particles()
    sim.sdf_snapshot(2.0, 2.0)                                                   # q + 1: plain
    sim.mesh_snapshot(2.0, 2.0)
    assert fs.lib.fluid_sdf_snapshot_attr(h, C.byref(prm), None) == ERR_STATE    # a third is refused, whatever its kind
    assert "two level-set snapshots" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_mesh_snapshot_attr(h, C.byref(prm), None) == ERR_STATE
    assert "two mesh snapshots" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_snapshot(h, C.byref(prm)) == ERR_STATE and fs.lib.fluid_mesh_snapshot(h, C.byref(prm)) == ERR_STATE
    g1, a1, g2, a2 = fs.SdfGridC(), fs.SdfAttrC(), fs.SdfGridC(), fs.SdfAttrC()
    m1, ma1, m2, ma2 = fs.MeshC(), fs.MeshAttrC(), fs.MeshC(), fs.MeshAttrC()
    assert fs.lib.fluid_sdf_wait_attr(h, C.byref(g1), C.byref(a1)) == 0 and fs.lib.fluid_sdf_wait_attr(h, C.byref(g2), C.byref(a2)) == 0
    assert fs.lib.fluid_mesh_wait_attr(h, C.byref(m1), C.byref(ma1)) == 0 and fs.lib.fluid_mesh_wait_attr(h, C.byref(m2), C.byref(ma2)) == 0
    # the _attr waits on the plain snapshots: geometry, NULL attributes
    assert g2.n_leaves > 0 and g2.values and (a2.n_leaves, a2.id, a2.velocity) == (g2.n_leaves, None, None)
    assert m2.n_vertices > 0 and m2.vertices and (ma2.n_vertices, ma2.velocity) == (m2.n_vertices, None)
    assert sim.sdf_stats()["bytes_to_host"] == g2.n_leaves * LEAF + 4
    assert sim.mesh_stats()["bytes_to_host"] == 12 * m2.n_vertices + 16 * m2.n_quads + 8
    # snapshot q's pointers are intact after snapshot q + 1 and all four waits
    r1 = reference(p1, v1, n, R, w, dx)
    k = g1.n_leaves
    org, lv, la = sdf_ref.leaf_list(r1[0], r1[1], sdf_ref.constants(R, w, dx)[3])
    li, lvel = attr_ref.leaf_attr(r1[2], r1[3], org)
    view = lambda p, t, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=shape)   # noqa: E731
    assert k == len(org) == a1.n_leaves and np.array_equal(view(g1.origin, C.c_int32, (k, 3)), org)
    assert np.array_equal(view(g1.values, C.c_uint32, (k, 512)), u32(lv))
    assert np.array_equal(view(a1.id, C.c_uint32, (k, 512)), li) and np.array_equal(view(a1.velocity, C.c_uint32, (k, 3, 512)), u32(lvel))
    nv = m1.n_vertices
    assert nv == len(r1[4]) == ma1.n_vertices and np.array_equal(view(m1.vertices, C.c_uint32, (nv, 3)), u32(r1[6][0]))
    assert np.array_equal(view(m1.quads, C.c_uint32, (m1.n_quads, 4)), r1[6][1])
    assert np.array_equal(view(ma1.velocity, C.c_uint32, (nv, 3)), u32(r1[4]))
    r2 = mesh_ref.mesh(sdf_ref.closed(p2, n, 2.0, 2.0, 1.0)[0])
    assert np.array_equal(view(m2.vertices, C.c_uint32, (m2.n_vertices, 3)), u32(r2[0]))
    # plain waits on attribute snapshots: the geometry alone, the slots reused in both orders
    for kind in ("attr", "plain", "attr", "attr", "plain"):
        sim.step()
        p, v = sim.download_particles()
        sim.sdf_snapshot(R, w, attr=kind == "attr")
        sim.mesh_snapshot(R, w, attr=kind == "attr")
        gg = sim.sdf_wait()
        vert, quads = sim.mesh_wait()
        val, act = sdf_ref.closed(p, n, R, w, dx)
        org, lv, la = sdf_ref.leaf_list(val, act, sdf_ref.constants(R, w, dx)[3])
        assert np.array_equal(gg.origin, org) and np.array_equal(u32(gg.values), u32(lv)) and np.array_equal(gg.active, la), kind
        mr = mesh_ref.mesh(val)
        assert np.array_equal(u32(vert), u32(mr[0])) and np.array_equal(quads, mr[1]), kind
        assert sim.sdf_stats()["bytes_to_host"] == len(org) * (LEAF + (ATTR if kind == "attr" else 0)) + 4
    sim.close()


def test_attribute_snapshots_do_not_disturb_the_steps(fs):
    """A handle that takes attribute snapshots after every step and one that never does end 3 steps with equal particles and stats."""
    n, (R, w, _) = 32, SETS[0]
    pos = fs.water_cube_drop(n, 8, seed=3)
    a, b = fs.FluidSim(n=n), fs.FluidSim(n=n)
    for s in (a, b):
        s.upload_particles(pos)
    sa, sb = [], []
    for k in range(3):
        sa.append(a.step())
        sb.append(b.step())
        b.sdf_snapshot(R, w, attr=True)
        b.mesh_snapshot(R, w, smooth=(1, 1, -0.25), attr=True)
        g, at = b.sdf_wait_attr()
        v, q, vv = b.mesh_wait_attr()
        assert g.n_leaves > 0 and at is not None and len(v) > 0 and vv.shape == v.shape
    assert sa == sb
    (pa, va), (pb, vb) = a.download_particles(), b.download_particles()
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    a.close()
    b.close()


def test_decomposed_handle_refuses(fs):
    fd = fs.load_dist()
    n = 16
    grp = fd.LocalGroup(1)
    sim = fd.DistFluidSim(n, (1, 1, 1), fd.uniform_cuts(n, (1, 1, 1)), grp.comms[0])
    h = sim._h
    prm = fs.SdfParams(1.5, 2.5)
    g, a, m, ma = fs.SdfGridC(), fs.SdfAttrC(), fs.MeshC(), fs.MeshAttrC()
    assert fs.lib.fluid_sdf_snapshot_attr(h, C.byref(prm), None) == ERR_STATE
    assert "single-GPU" in fs.lib.fluid_last_error().decode()
    assert fs.lib.fluid_sdf_wait_attr(h, C.byref(g), C.byref(a)) == ERR_STATE
    assert fs.lib.fluid_mesh_snapshot_attr(h, C.byref(prm), None) == ERR_STATE
    assert fs.lib.fluid_mesh_wait_attr(h, C.byref(m), C.byref(ma)) == ERR_STATE
    sim.close()


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii")
    nv = int(head.split("element vertex ")[1].split("\n")[0])
    nq = int(head.split("element face ")[1].split("\n")[0])
    k = 6 if "property float vx\n" in head else 3
    v = np.frombuffer(raw, "<f4", k * nv, end).reshape(nv, k)
    f = np.frombuffer(raw, np.dtype([("k", "u1"), ("i", "<u4", 4)]), nq, end + 4 * k * nv)
    assert end + 4 * k * nv + 17 * nq == len(raw)
    return v, f


def test_driver_writes_the_velocities(fs, tmp_path):
    """The `fluid` program with FLUID_OUT_MESH and FLUID_OUT_MESH_VEL=SCALE: mesh<i>.ply re-reads with six floats per vertex, its
    positions and faces are those of a run without the switch, its velocities the handle's of the same scene times SCALE, and
    stdout and every other file are what they are without it."""
    import leaf_ref
    n, ppc, steps, (R, w, dx), scale = 24, 4, 2, SETS[0], 0.5
    exe = os.path.join(ROOT, "fluid-simulation_amd", "fluid")
    outs = {}
    for mode in ("mesh", "vel"):
        d = tmp_path / mode
        d.mkdir()
        env = dict(os.environ, FLUID_N=str(n), FLUID_PPC=str(ppc), FLUID_STEPS=str(steps), FLUID_OUT=str(d / "simulation"), FLUID_OUT_MESH=f"{R},{w}")
        for k in ("FLUID_OUT_MESH_VEL", "FLUID_OUT_SURFACE", "FLUID_OUT_DENSE", "FLUID_BLOCKS", "FLUID_BLOCKS_SURFACE", "FLUID_SOURCE_EVERY", "FLUID_RAW",
                  "FLUID_OUT_SMOOTH"):
            env.pop(k, None)
        if mode == "vel":
            env["FLUID_OUT_MESH_VEL"] = str(scale)
        r = subprocess.run([exe], capture_output=True, text=True, env=env, cwd=d, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = [ln for ln in r.stdout.splitlines() if not ln.startswith("Time Taken")]
    assert outs["mesh"] == outs["vel"]
    names = lambda m: sorted(str(p.relative_to(tmp_path / m)) for p in (tmp_path / m).rglob("*") if p.is_file())   # noqa: E731
    assert names("mesh") == names("vel")
    for nm in names("mesh"):
        if not nm.endswith(".ply"):
            assert leaf_ref.same_file(tmp_path / "mesh" / nm, tmp_path / "vel" / nm), nm
    sim = fs.FluidSim(n=n)
    sim.upload_particles(fs.water_cube_drop(n, ppc, seed=0))
    for i in range(steps):
        sim.step()
        sim.mesh_snapshot(R, w, attr=True)
        v, q, vv = sim.mesh_wait_attr()
        pv, pf = read_ply(tmp_path / "mesh" / f"simulation/mesh{i}.ply")
        av, af = read_ply(tmp_path / "vel" / f"simulation/mesh{i}.ply")
        assert pv.shape[1] == 3 and av.shape[1] == 6 and len(q) > 0
        assert np.array_equal(u32(av[:, :3]), u32(pv)) and np.array_equal(af, pf), i
        assert np.array_equal(u32(pv), u32(v * np.float32(dx))) and np.array_equal(pf["i"], q), i
        assert np.array_equal(u32(av[:, 3:]), u32(vv * np.float32(scale))) and np.abs(vv).max() > 0, i
    sim.close()
