"""CPU (-m "not gpu"): the numpy references of the liquid-surface pipeline (sdf_filter_ref, sdf_track_ref, sdf_weno_ref, sdf_flow_ref)
and the host library (fluid_sdf_filter, fluid_sdf_filter_tracked, fluid_sdf_flow) against OpenVDB's own operators, compiled in
place over a mock dense grid (oracle/vdb_ref.cpp -> oracle/_ref/libvdb_ref.so; skipped where that library was not built).  Every
comparison is on uint32 views; there is no tolerance anywhere.  The fields are those of tests/vdb_cases.py: the unfiltered scenes,
and six adversarial fields no particle set gives.  tests/golden/vdb_passes.npz (written by tests/golden/make_vdb_golden.py from the
library) holds a part of this for the machines without the reference: the numpy files and the host library reproduce it without
the library, and the library reproduces it where it is built, so that a stale fixture shows.

Changed-voxel rule: every case must change more than half of its active voxels unless the operator is null on the field by
construction (FLAT below says which and why, and null_reason_holds() asserts the reason); those cases are still compared bit for bit.
"""
import os
import sys

import numpy as np
import pytest

import mesh_ref
import sdf_filter_ref
import sdf_flow_ref
import sdf_ref
import sdf_track_ref
import sdf_weno_ref
import vdb_cases as VC
from test_sdf_weno_ref import septuples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import vdb_ref  # noqa: E402

REF = vdb_ref.ref
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref/libvdb_ref.so not built (needs the reference tree)")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vdb_passes.npz")
F = np.float32
u32 = VC.u32
COLUMNS = 10648                                            # 22^3 >= 10 000: the centres of the first-order grid below

# name -> (numpy pass, OpenVDB pass), both (val, act, bg, dx) -> val
PASSES = {
    "first": (lambda v, a, bg, dx: sdf_track_ref.norm_pass(v, a, bg, dx), lambda v, a, bg, dx: REF.norm_pass(v, a, bg, dx, VC.FIRST)),
    "hjweno5": (lambda v, a, bg, dx: sdf_weno_ref.norm_pass_weno(v, a, bg, dx), lambda v, a, bg, dx: REF.norm_pass(v, a, bg, dx, VC.HJWENO5)),
    "laplacian": (lambda v, a, bg, dx: sdf_flow_ref.laplacian_pass(v, a, bg, dx), lambda v, a, bg, dx: REF.laplacian_pass(v, a, bg, dx)),
    "curvature": (lambda v, a, bg, dx: sdf_flow_ref.curvature_pass(v, a, bg, dx), lambda v, a, bg, dx: REF.curvature_pass(v, a, bg, dx)),
}
for _w in (1, 2):
    PASSES[f"median{_w}"] = (lambda v, a, bg, dx, w=_w: sdf_flow_ref.median_pass(v, a, bg, w), lambda v, a, bg, dx, w=_w: REF.median_pass(v, a, bg, w))
for _w in (1, 2, 4):
    for _ax in range(3):
        PASSES[f"box{_w}axis{_ax}"] = (lambda v, a, bg, dx, w=_w, ax=_ax: sdf_filter_ref.box_pass(v, a, bg, w, ax),
                                       lambda v, a, bg, dx, w=_w, ax=_ax: REF.box_pass(v, a, bg, w, ax))
_SMOOTHING = tuple(k for k in PASSES if k not in ("first", "hjweno5"))
# The cases where the operator is null on most of the field by construction, so that "more than half change" cannot be asked.  Each
# reason is asserted by null_reason_holds() below, so that an exemption cannot hide a pass that does nothing:
FLAT = {
    # 70 % of the voxels hold 0.75: it is the median of most cubes, and most voxels hold it already
    "flat": ("median1", "median2"),
    # an affine field is a fixed point of every smoothing pass (second differences vanish, the median and the mean of a symmetric
    # cube are its centre); only voxels that read the background beyond the grid move.  Its gradient is not 1: both normalisations
    # move it
    "linear": _SMOOTHING,
    # values of 1e-20 give a squared gradient of 1e-40, under Tolerance<double> = 1e-15: the curvature's null branch, which is
    # what the field is for
    "tiny": ("curvature",),
    # at 1e18 WENO5's smoothness terms are near 1e76 in double, its weights near 1e-77, and the weighted sum, narrowed to float32
    # before the division (math/FiniteDifference.h:345), underflows: every biased difference is exactly 0, the gradient term
    # vanishes, and the step left, at most 0.3 dx, is under the spacing of float32 at 1e18
    "huge": ("hjweno5",),
}


def reach_of(name):
    """How far a smoothing pass reads along each axis."""
    if name.startswith("box"):
        r = [0, 0, 0]
        r[int(name[-1])] = int(name[3])
        return r
    return [int(name[6:])] * 3 if name.startswith("median") else [1, 1, 1]


def inside(n, reach):
    """The voxels whose stencil stays in the grid."""
    m = np.ones((n, n, n), bool)
    for a, r in enumerate(reach):
        idx = np.arange(n).reshape([-1 if i == a else 1 for i in range(3)])
        m &= (idx >= r) & (idx < n - r)
    return m


def null_reason_holds(field, name, val, act, bg, out):
    """The reason FLAT gives for (field, name), on the inputs and on OpenVDB's result `out`."""
    n = val.shape[0]
    same = u32(out) == u32(val)
    if field == "flat":
        assert (out[act] == F(0.75)).sum() * 2 > act.sum() and (val[act] == F(0.75)).sum() * 2 > act.sum()
    elif field == "linear":
        m = act & inside(n, reach_of(name))
        assert m.sum() > 100 and same[m].all(), (name, int((~same[m]).sum()))
        assert not same[act & ~m].all()                                # the pass is alive: at the rim it reads the background
    elif field == "tiny":   # math/Stencils.h:1545-1554 on the inputs: the squared central-difference gradient, in double
        P = np.pad(val, 1, constant_values=bg).astype(np.float64)
        g2 = sum((0.5 * (np.roll(P, -1, a) - np.roll(P, 1, a))[1:-1, 1:-1, 1:-1]) ** 2 for a in range(3))
        m = act & inside(n, [1, 1, 1])
        assert m.sum() > 100 and (g2[m] <= 1e-15).all() and same[m].all()
        assert (g2[act & ~m] > 1e-15).all() and not same[act & ~m].any()   # the rim reads bg: a gradient, and the voxel moves
    elif field == "huge":
        P = np.pad(val, 3, constant_values=bg)
        zero = np.ones((n, n, n), bool)
        for a in range(3):
            u = []
            for k in range(-3, 4):
                sl = [slice(3, n + 3)] * 3
                sl[a] = slice(3 + k, 3 + k + n)
                u.append(P[tuple(sl)].ravel())
            dm, dp = REF.axis_diffs(np.array(u))
            zero &= ((dm == 0) & (dp == 0)).reshape(n, n, n)
        assert (zero & act).sum() * 2 > act.sum() and same[zero & act].all()
        assert float(np.spacing(np.abs(val[zero & act]).min())) > 0.3 * 3     # 0.3 dx at dx <= 1, with room
    else:
        raise KeyError(field)


def check_passes(val, act, bg, dx, what, field=None):
    flat = FLAT.get(field, ())
    assert VC.clean(val), what
    n_act = int(act.sum())
    assert n_act > 100, what
    for name, (ours, theirs) in PASSES.items():
        with np.errstate(all="ignore"):
            a = ours(val, act, bg, dx)
        b = theirs(val, act, bg, dx)
        changed = int((u32(b) != u32(val))[act].sum())
        print(f"{what} {name}: {changed} of {n_act} active voxels change")
        assert np.array_equal(u32(a), u32(b)), (what, name, int((u32(a) != u32(b)).sum()))
        assert np.array_equal(u32(b)[~act], u32(val)[~act]), (what, name)
        if name not in flat:
            assert 2 * changed > n_act, (what, name, changed, n_act)
        else:
            null_reason_holds(field, name, val, act, bg, b)


# ---- functions -----------------------------------------------------------------------------------------------------------------
@needs_ref
def test_weno5_and_the_biased_differences_are_openvdbs():
    u = septuples(COLUMNS, 11)
    assert u.shape == (7, COLUMNS) and VC.clean(u)
    for s in (u[0:5], u[2:7], u[1:6][::-1]):
        assert np.array_equal(u32(sdf_weno_ref.weno5(*s)), u32(REF.weno5(*s)))
    dm, dp = sdf_weno_ref.axis_diffs(list(u))
    rm, rp = REF.axis_diffs(u)
    assert np.array_equal(u32(dm), u32(rm)) and np.array_equal(u32(dp), u32(rp))
    assert len(np.unique(u32(rm))) > COLUMNS // 2 and (u32(rm) != u32(rp)).sum() > COLUMNS // 2


def three_septuples(seed):
    ux, uy, uz = septuples(COLUMNS, seed), septuples(COLUMNS, seed + 1), septuples(COLUMNS, seed + 2)
    uy[3], uz[3] = ux[3], ux[3]
    return ux, uy, uz


@needs_ref
@pytest.mark.parametrize("dx", VC.DXS)
def test_the_hjweno5_voxel_step_is_openvdbs(dx):
    ux, uy, uz = three_septuples(21)
    v = sdf_weno_ref.voxel_value(ux, uy, uz, dx)
    r = REF.voxel_value(ux, uy, uz, dx, VC.HJWENO5)
    assert np.array_equal(u32(v), u32(r))
    assert (u32(r) != u32(ux[3])).sum() > COLUMNS // 2


def first_order_grid(ux, uy, uz):
    """A 66^3 grid of 22^3 voxels three apart, each with its own six neighbours: column c of the septuples around voxel c."""
    m = 22
    assert ux.shape[1] == m ** 3
    val = np.zeros((3 * m,) * 3, F)
    act = np.zeros(val.shape, bool)
    c = slice(1, None, 3)
    val[c, c, c] = ux[3].reshape(m, m, m)
    act[c, c, c] = True
    for axis, u in enumerate((ux, uy, uz)):
        for k, off in ((2, 0), (4, 2)):
            sl = [c, c, c]
            sl[axis] = slice(off, None, 3)
            val[tuple(sl)] = u[k].reshape(m, m, m)
    return val, act, c


@needs_ref
@pytest.mark.parametrize("dx", VC.DXS)
def test_the_first_order_voxel_step_is_openvdbs(dx):
    ux, uy, uz = three_septuples(31)
    val, act, c = first_order_grid(ux, uy, uz)
    v = sdf_track_ref.norm_pass(val, act, 3 * dx, dx)[c, c, c].ravel()
    r = REF.voxel_value(ux, uy, uz, dx, VC.FIRST)
    assert np.array_equal(u32(v), u32(r))
    assert np.array_equal(u32(REF.norm_pass(val, act, 3 * dx, dx, VC.FIRST)[c, c, c].ravel()), u32(r))   # the library's two ways agree
    assert (u32(r) != u32(ux[3])).sum() > COLUMNS // 2


@needs_ref
@pytest.mark.parametrize("dx", VC.DXS + (0.3,))
def test_time_steps_are_openvdbs(dx):
    dt, inv, dt_lap, dt_curv = REF.consts(dx)
    _, lap, curv = sdf_flow_ref.consts(dx)
    assert u32(lap) == u32(dt_lap) and u32(curv) == u32(dt_curv)
    assert u32(F(dx) * F(0.3)) == u32(dt) and u32(F(1) / F(dx)) == u32(inv)            # what sdf_track_ref.norm_pass states


# ---- passes ----------------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("R,w,dx", mesh_ref.SETS)
@pytest.mark.parametrize("name,n", VC.SCENES)
def test_every_pass_on_the_scenes_is_openvdbs(name, n, R, w, dx):
    val, act, bg = VC.scene_field(name, n, R, w, dx)
    check_passes(val, act, bg, dx, f"{name} {n} {(R, w, dx)}")


@needs_ref
@pytest.mark.parametrize("dx", VC.DXS)
@pytest.mark.parametrize("field", VC.ADVERSARIAL)
def test_every_pass_on_the_adversarial_fields_is_openvdbs(field, dx):
    val, act, bg = VC.adversarial(14, dx)[field]
    assert 0.8 < act.mean() < 0.9
    check_passes(val, act, bg, dx, f"{field} dx={dx}", field)
    if field == "flat":   # math/Stencils.h:1545-1554 on the inputs: the voxels whose central-difference gradient is under Tolerance<double>
        P = np.pad(val, 1, constant_values=bg).astype(np.float64)
        g2 = sum((0.5 * (np.roll(P, -1, a) - np.roll(P, 1, a))[1:-1, 1:-1, 1:-1]) ** 2 for a in range(3))
        assert (act & (g2 <= 1e-15)).sum() > 50


@needs_ref
@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("field", ["rough", "integer"])
def test_median_of_a_cube_is_openvdbs(field, W):
    """sdf_flow_ref.median_of, the one-voxel statement of the rank: the cube of every 13th voxel, gathered here, against
    BaseStencil::median of the DenseStencil at that voxel."""
    val, act, bg = VC.adversarial(14, 1.0)[field]
    n = val.shape[0]
    P = np.pad(val, W, constant_values=bg)
    r = REF.median_pass(val, np.ones_like(act), bg, W)
    idx = np.arange(0, n ** 3, 13)
    mine = [sdf_flow_ref.median_of(P[i:i + 2 * W + 1, j:j + 2 * W + 1, k:k + 2 * W + 1]) for i, j, k in zip(*np.unravel_index(idx, val.shape))]
    assert np.array_equal(u32(np.array(mine, F)), u32(r.ravel()[idx]))
    assert (u32(r.ravel()[idx]) != u32(val.ravel()[idx])).sum() > len(idx) // 4


@needs_ref
def test_median_of_an_even_count_takes_openvdbs_rank():
    """27 and 125 are odd, and (m - 1) >> 1 == m >> 1 for an odd m: the rank shows only on an even count.  BaseStencil::median over the
    eight values of OpenVDB's BoxStencil against median_of of the same eight."""
    val, act, bg = VC.adversarial(14, 1.0)["rough"]
    n = val.shape[0]
    P = np.pad(val, ((0, 1),) * 3, constant_values=bg)
    r = REF.median_of_eight(val, np.ones_like(act), bg)
    mine = np.array([sdf_flow_ref.median_of(P[i:i + 2, j:j + 2, k:k + 2]) for i, j, k in np.ndindex(n, n, n)], F)
    assert np.array_equal(u32(mine), u32(r.ravel()))
    upper = np.array([np.sort(P[i:i + 2, j:j + 2, k:k + 2].ravel())[4] for i, j, k in np.ndindex(n, n, n)], F)
    assert (u32(upper) != u32(r.ravel())).sum() > n ** 3 // 2                            # the other middle rank is another value


# ---- composition -------------------------------------------------------------------------------------------------------------------
@needs_ref
def test_box_order_is_openvdbs():
    passes, names = REF.box_order()
    assert names == (0, 2, 1)                              # boxX averages along 0, boxY along 2, boxZ along 1
    assert passes == (0, 2, 1) == tuple(sdf_filter_ref.ORDER)


OFFSETS = (0.0, 0.0005, -0.0005, 0.25, -0.25, 0.5, -0.5, 0.6, -0.6, 1.0, -1.0, 1.3, -1.3, 2.0, -2.0)


@needs_ref
@pytest.mark.parametrize("dx", (1.0, 0.5, 0.3))
def test_offset_steps_are_openvdbs(dx):
    for units in OFFSETS:
        off = F(units) * F(dx)
        a, b = sdf_track_ref.offset_steps(off, dx), REF.offset_steps(off, dx)
        assert len(a) == len(b) and np.array_equal(u32(np.array(a, F)), u32(np.array(b, F))), (units, a, b)
        if abs(units) <= 0.0005:
            assert len(b) == 0                             # below 0.001 CFL: no step at all
        else:
            assert len(b) >= 1 and abs(float(np.sum(b, dtype=np.float64)) - float(off)) <= 0.001 * 0.5 * dx + 1e-6


# ---- the host library ----------------------------------------------------------------------------------------------------------------
KINDS = [(VC.BOX, 1), (VC.BOX, 2), (VC.MEDIAN, 1), (VC.MEDIAN, 2), (VC.LAPLACIAN, 1), (VC.CURVATURE, 1)]
TRACKS = [None, (1, False, "first"), (1, False, "hjweno5")]


def host_grid(fs, val, act, bg):
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    return fs.SdfGrid(val.shape[0], org, v, a, bg, 1.0, 3.0)   # half_width 3: bg = 3 dx


def host_is(fs, g, kind, W, track, exp, bg, what):
    """fluid_sdf_flow — and for the box filter the two older entry points — with K = 1 give the dense (val, act) `exp`."""
    org, v, a = sdf_ref.leaf_list(exp[0], exp[1], bg)
    outs = [fs.sdf_flow(g, kind, (W, 1, 0.0), track=track)]
    if kind == VC.BOX:
        outs.append(fs.sdf_filter(g, W, 1, 0.0) if track is None else fs.sdf_filter_tracked(g, (W, 1, 0.0), track)[0])
    for out in outs:
        assert out.n_leaves == len(org) and np.array_equal(out.origin, org), what
        assert np.array_equal(out.active, a), what
        assert np.array_equal(u32(out.values), u32(v)), (what, int((u32(out.values) != u32(v)).sum()))


@needs_ref
@pytest.mark.parametrize("dx", VC.DXS)
@pytest.mark.parametrize("field", VC.ADVERSARIAL)
def test_host_library_on_adversarial_lists_is_openvdbs(fs, field, dx):
    val, act, bg = VC.adversarial(16, dx)[field]
    val = VC.as_list_field(val, act, bg)
    g = host_grid(fs, val, act, bg)
    assert g.n_leaves == 8
    for kind, W in KINDS:
        for track in TRACKS:
            N, scheme = (0, VC.FIRST) if track is None else (track[0], VC.HJWENO5 if track[2] == "hjweno5" else VC.FIRST)
            exp = VC.flow(REF, kind, val, act, bg, dx, W, 1, N, False, scheme)
            host_is(fs, g, kind, W, track, exp, bg, f"{field} dx={dx} kind={kind} W={W} track={track}")


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN)


def golden_ops(z, field):
    """(name, (val, act, bg, dx) -> val by the numpy files, the stored active values) of every stored operation."""
    for name, (ours, _) in PASSES.items():
        key = f"{field}_{name}"
        if key in z.files:
            yield name, ours, z[key]


def test_numpy_references_reproduce_the_fixture():
    z = golden()
    dx = float(z["dx"])
    for field in ("rough", "integer"):
        val, act, bg = z[f"{field}_val"], z[f"{field}_act"].astype(bool), z["bg"]
        seen = 0
        for name, ours, stored in golden_ops(z, field):
            assert np.array_equal(u32(ours(val, act, bg, dx)[act]), u32(stored)), (field, name)
            seen += 1
        assert seen == 7
        it = sdf_filter_ref.smooth(val, act, bg, 1, 1)                                   # the three passes in ORDER
        assert np.array_equal(u32(it[act]), u32(z[f"{field}_iter_box1"])), field
        for scheme, nm in ((sdf_weno_ref.FIRST, "first"), (sdf_weno_ref.HJWENO5, "hjweno5")):
            tv, _ = sdf_weno_ref.track(it, act, bg, dx, 1, False, scheme)
            assert np.array_equal(u32(tv[act]), u32(z[f"{field}_iter_box1_{nm}"])), (field, nm)
    u = z["septuples"]
    assert np.array_equal(u32(sdf_weno_ref.weno5(*u[0:5])), u32(z["sept_weno5"]))
    dm, dp = sdf_weno_ref.axis_diffs(list(u))
    assert np.array_equal(u32(dm), u32(z["sept_dm"])) and np.array_equal(u32(dp), u32(z["sept_dp"]))
    ux, uy, uz = z["sept_ux"], z["sept_uy"], z["sept_uz"]
    assert np.array_equal(u32(sdf_weno_ref.voxel_value(ux, uy, uz, dx)), u32(z["sept_voxel_hjweno5"]))
    for units, steps in zip(z["offset_units"], np.split(z["offset_steps"], np.cumsum(z["offset_counts"])[:-1])):
        mine = np.array(sdf_track_ref.offset_steps(F(units) * F(dx), dx), F)
        assert np.array_equal(u32(mine), u32(steps)), units
    assert tuple(z["box_order"]) == tuple(sdf_filter_ref.ORDER)


def test_host_library_reproduces_the_fixture(fs):
    z = golden()
    for field in ("rough", "integer"):
        val, act, bg = z[f"{field}_val"], z[f"{field}_act"].astype(bool), z["bg"]
        g = host_grid(fs, val, act, bg)
        assert g.n_leaves > 0

        def dense(key):
            out = np.array(val)
            out[act] = z[f"{field}_{key}"]
            return out, act

        for key, kind, W in (("median1", VC.MEDIAN, 1), ("median2", VC.MEDIAN, 2), ("laplacian", VC.LAPLACIAN, 1), ("curvature", VC.CURVATURE, 1)):
            host_is(fs, g, kind, W, None, dense(key), bg, (field, key))
        host_is(fs, g, VC.BOX, 1, None, dense("iter_box1"), bg, (field, "box"))
        host_is(fs, g, VC.BOX, 1, (1, False, "first"), dense("iter_box1_first"), bg, (field, "box, first"))
        host_is(fs, g, VC.BOX, 1, (1, False, "hjweno5"), dense("iter_box1_hjweno5"), bg, (field, "box, hjweno5"))


@needs_ref
def test_library_reproduces_the_fixture():
    """A fixture that no longer is what OpenVDB's lines give shows here: rewrite it with tests/golden/make_vdb_golden.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_vdb_golden
    z, fresh = golden(), make_vdb_golden.arrays(REF)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        a, b = z[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b), k
