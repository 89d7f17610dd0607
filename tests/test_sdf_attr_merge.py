"""Host only: fluid_sdf_attr_grids_merge (include/fluid_hip.h, "liquid surface, attributes (decomposed runs)") against
tests/attr_merge_ref.py.  The parts are the rank records of subsets of a particle set with given ids, the expected merge is the
reference of the whole set: origins, masks, value bits, ids and velocity bits must be equal exactly, and the geometry must be
fluid_sdf_grids_merge's.  Random scenes do not reach the voxels where a merge that looks at values or at part order goes wrong;
the two scenes that do are built on purpose and the test first counts those voxels for itself."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_merge_ref
import attr_ref
import sdf_ref
from sdf_testlib import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid-simulation_amd", "csrc")
SETS = [(1.5, 2.5, 1.0), (3.0, 1.0, 1.0)]                 # (R, w, dx): SETS of test_gpu_dist_sdf.py
ERR_ARG = 1
NO_ID = 0xFFFFFFFF
FILL = 0x5A


def particles(n):
    """test_sdf_merge.py's set: a filled block of 8 per cell round the centre and 150 scattered points, some outside the grid."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    rng = np.random.default_rng(100 + n)
    c = np.stack(np.meshgrid(*[np.arange(-2, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    block = np.repeat(c, 8, axis=0) + rng.uniform(-0.49, 0.49, (8 * len(c), 3))
    return np.vstack([block, rng.uniform(lo - 1.0, hi + 1.0, (150, 3))])


def objects(fs, rec, n, R, w, dx):
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    return (fs.SdfGrid(n, rec["origin"], rec["values"], rec["active"], bg, fR, fw),
            fs.SdfAttrPart(rec["id"], rec["velocity"], rec["dist2"]))


def split_rows(pos, n):
    """Rows of the parts of every split."""
    rng = np.random.default_rng(7 + n)
    half = rng.integers(0, 2, len(pos))
    k5 = rng.integers(0, 5, len(pos))
    k5[k5 == 3] = 0                                                        # one part of the five is empty
    oct_ = ((sdf_ref.base_cell(pos) >= 0) * np.array([4, 2, 1])).sum(axis=1)
    rows = np.arange(len(pos))
    return {"half": [rows[half == i] for i in range(2)], "by_x": [rows[pos[:, 0] < 0], rows[pos[:, 0] >= 0]],
            "eight": [rows[oct_ == i] for i in range(8)], "with_empty": [rows[k5 == i] for i in range(5)], "single": [rows]}


_CASES = {}


def case(fs, n, si):
    """(pos, vel, ids, reference of the union, {split: [(SdfGrid, SdfAttrPart)]}), computed once per (n, set), never modified."""
    if (n, si) not in _CASES:
        R, w, dx = SETS[si]
        pos = particles(n)
        vel = attr_ref.velocities(pos)
        ids = np.random.default_rng(3).permutation(len(pos)).astype(np.uint32) * 3 + 5      # ids are no rows
        whole = attr_merge_ref.merged(pos, vel, ids, n, R, w, dx)
        memo = {}

        def part(rows):
            key = rows.tobytes()
            if key not in memo:
                memo[key] = objects(fs, attr_merge_ref.rank_record(pos[rows], vel[rows], ids[rows], n, R, w, dx), n, R, w, dx)
            return memo[key]
        _CASES[(n, si)] = (pos, vel, ids, whole, {name: [part(r) for r in rs] for name, rs in split_rows(pos, n).items()})
    return _CASES[(n, si)]


def equals(grid, attr, ref):
    return (np.array_equal(grid.origin, ref["origin"]) and np.array_equal(grid.active, ref["active"]) and
            np.array_equal(u32(grid.values), u32(ref["values"])) and np.array_equal(attr.id, ref["id"]) and
            np.array_equal(u32(attr.velocity), u32(ref["velocity"])))


@pytest.mark.parametrize("split", ["half", "by_x", "eight", "with_empty", "single"])
@pytest.mark.parametrize("si", range(2))
@pytest.mark.parametrize("n", [16, 25])
def test_merge_equals_the_whole_set(fs, n, si, split):
    _, _, _, whole, parts = case(fs, n, si)
    ps = parts[split]
    if split == "with_empty":
        assert ps[3][0].n_leaves == 0
    grid, attr = fs.merge_sdf_attr_grids([g for g, _ in ps], [a for _, a in ps])
    assert grid.n_leaves == len(whole["origin"]) > 0
    assert equals(grid, attr, whole)
    plain = fs.merge_sdf_grids([g for g, _ in ps])                          # the geometry is the plain merge's, byte for byte
    assert grid.origin.tobytes() == plain.origin.tobytes() and grid.values.tobytes() == plain.values.tobytes()
    assert np.array_equal(grid.active, plain.active)
    assert ((attr.id != NO_ID) == grid.active).all()
    if split != "single":
        both = sum(len(set(map(tuple, g.origin.tolist())) & set(map(tuple, ps[0][0].origin.tolist()))) for g, _ in ps[1:])
        assert both > 0                                                    # leaves that several parts list


BUILT = {"near": np.array([[-2.75 - 2e-7, 0.1, 0.2], [2.75, 0.1, 0.2]]), "tie": np.array([[-2.75, 0.1, 0.2], [2.75, 0.1, 0.2]])}
BUILT_VEL = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.125]])


def built_records(scene, n, R, w, dx, ids):
    """The records of the left and of the right particle of a built scene, with ids[0] and ids[1]."""
    pos = BUILT[scene]
    return [attr_merge_ref.rank_record(pos[i:i + 1], BUILT_VEL[i:i + 1], [ids[i]], n, R, w, dx) for i in range(2)]


def shared_voxels(ra, rb):
    """Per leaf both records list: (origin, active in both, value bits equal, dist2 of a, dist2 of b)."""
    a = {tuple(o): k for k, o in enumerate(ra["origin"].tolist())}
    for k, o in enumerate(map(tuple, rb["origin"].tolist())):
        if o in a:
            j = a[o]
            yield (o, ra["active"][j] & rb["active"][k], u32(ra["values"][j]) == u32(rb["values"][k]), ra["dist2"][j], rb["dist2"][k])


@pytest.mark.parametrize("R,w,dx", SETS)
def test_equal_values_do_not_imply_equal_distances(fs, R, w, dx):
    """The near mirror: the farther (left) particle has id 0 and is part 0.  On some voxels both parts are active with the same
    value bits although the right particle is strictly closer: "the first part on equal values" picks the wrong particle there."""
    n = 16
    left, right = built_records("near", n, R, w, dx, (0, 1))
    count, where = 0, []
    for o, both, same_val, da, db in shared_voxels(left, right):
        hit = both & same_val & (da != db)
        assert (db[hit] < da[hit]).all()                                   # the right particle is the closer one on every such voxel
        count += int(hit.sum())
        where.append((o, hit))
    print(f"R={R} w={w}: voxels active in both parts with bit-equal values and different dist2: {count}")
    assert count == 13
    grid, attr = fs.merge_sdf_attr_grids(*zip(*[objects(fs, r, n, R, w, dx) for r in (left, right)]))
    assert equals(grid, attr, attr_merge_ref.merged(BUILT["near"], BUILT_VEL, [0, 1], n, R, w, dx))
    at = {tuple(o): k for k, o in enumerate(grid.origin.tolist())}
    for o, hit in where:
        assert (attr.id[at[o]][hit] == 1).all()
        assert (u32(attr.velocity[at[o]][:, hit]) == u32(BUILT_VEL[1].astype(np.float32))[:, None]).all()


@pytest.mark.parametrize("R,w,dx", SETS)
def test_equal_distances_give_the_smaller_id_whichever_part_holds_it(fs, R, w, dx):
    """The exact mirror: the voxels of the plane x = 0 tie on dist2 itself.  The smaller id is held by the LATER part."""
    n = 16
    left, right = built_records("tie", n, R, w, dx, (7, 3))                # part 0 holds id 7, part 1 holds id 3
    count, where = 0, []
    for o, both, _, da, db in shared_voxels(left, right):
        hit = both & (da == db)
        count += int(hit.sum())
        where.append((o, hit))
    print(f"R={R} w={w}: voxels active in both parts with equal dist2: {count}")
    assert count == 24
    grid, attr = fs.merge_sdf_attr_grids(*zip(*[objects(fs, r, n, R, w, dx) for r in (left, right)]))
    assert equals(grid, attr, attr_merge_ref.merged(BUILT["tie"], BUILT_VEL, [7, 3], n, R, w, dx))
    at = {tuple(o): k for k, o in enumerate(grid.origin.tolist())}
    for o, hit in where:
        assert (attr.id[at[o]][hit] == 3).all()
    # the same parts in the other order, and the same id on both parts: the first part
    g2, a2 = fs.merge_sdf_attr_grids(*zip(*[objects(fs, r, n, R, w, dx) for r in (right, left)]))
    assert equals(g2, a2, dict(origin=grid.origin, values=grid.values, active=grid.active, id=attr.id, velocity=attr.velocity))
    l7, r7 = built_records("tie", n, R, w, dx, (7, 7))
    g3, a3 = fs.merge_sdf_attr_grids(*zip(*[objects(fs, r, n, R, w, dx) for r in (l7, r7)]))
    for o, hit in where:
        k = at[o]
        assert (a3.id[k][hit] == 7).all() and (u32(a3.velocity[k][:, hit]) == u32(BUILT_VEL[0].astype(np.float32))[:, None]).all()


def raw_merge(fs, pairs, cap, count_only=False, attrs=None, n_parts=None):
    """(return value, the five output arrays pre-filled with FILL) of the C call on [(SdfGrid, SdfAttrPart)]."""
    cs = [g._c() for g, _ in pairs]
    arr = (fs.SdfGridC * len(pairs))(*[c for c, _ in cs])
    aarr = attrs if attrs is not None else (fs.SdfAttrPartC * len(pairs))(*[a._c() for _, a in pairs])
    n_parts = len(pairs) if n_parts is None else n_parts
    if count_only:
        return fs.lib.fluid_sdf_attr_grids_merge(arr, aarr, n_parts, cap, None, None, None, None, None), None
    room = max(cap, 1)
    outs = [np.full((room, 3), FILL, np.int32), np.full((room, 512), FILL, np.float32), np.full((room, 8), FILL, np.uint64),
            np.full((room, 512), FILL, np.uint32), np.full((room, 3, 512), FILL, np.float32)]
    k = fs.lib.fluid_sdf_attr_grids_merge(arr, aarr, n_parts, cap, *[x.ctypes.data_as(C.c_void_p) for x in outs])
    return k, outs


def untouched(outs):
    return all((x == x.dtype.type(FILL)).all() for x in outs)


def test_counts_capacity_single_and_empty(fs):
    n = 16
    _, _, _, whole, parts = case(fs, n, 1)
    ps = parts["eight"]
    k = len(whole["origin"])
    assert raw_merge(fs, ps, 0, count_only=True)[0] == k
    assert raw_merge(fs, ps, 123456, count_only=True)[0] == k              # cap_leaves is ignored
    r, outs = raw_merge(fs, ps, k - 1)
    assert r == -ERR_ARG and untouched(outs)                               # a cap that is too small writes nothing
    r, outs = raw_merge(fs, ps, k)
    assert r == k and np.array_equal(outs[0], whole["origin"]) and np.array_equal(outs[3], whole["id"])
    g5, a5 = ps[5]
    g, a = fs.merge_sdf_attr_grids([g5], [a5])                             # one part alone: that part
    assert equals(g, a, dict(origin=g5.origin, values=g5.values, active=g5.active, id=a5.id, velocity=a5.velocity))
    eg = fs.SdfGrid(n, np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 512), bool), g5.background, g5.radius,
                    g5.half_width)
    ea = fs.SdfAttrPart(np.empty((0, 512), np.uint32), np.empty((0, 3, 512), np.float32), np.empty((0, 512), np.float32))
    g, a = fs.merge_sdf_attr_grids([eg, eg, eg], [ea, ea, ea])
    assert g.n_leaves == 0 and a.n_leaves == 0
    g, a = fs.merge_sdf_attr_grids([eg, g5, eg], [ea, a5, ea])
    assert equals(g, a, dict(origin=g5.origin, values=g5.values, active=g5.active, id=a5.id, velocity=a5.velocity))
    c = fs.SdfGridC(n, 0, g5.background, g5.radius, g5.half_width, None, None, None)        # NULL pointers behind no leaves
    ac = fs.SdfAttrPartC(0, None, None, None)
    assert fs.lib.fluid_sdf_attr_grids_merge((fs.SdfGridC * 2)(c, c), (fs.SdfAttrPartC * 2)(ac, ac), 2, 0, *[None] * 5) == 0
    r, outs = raw_merge(fs, [(eg, ea), (eg, ea)], 4)
    assert r == 0 and untouched(outs)


def test_refusals_leave_the_output_alone(fs):
    n = 16
    _, _, _, whole, parts = case(fs, n, 1)
    (a, aa), (b, ba) = parts["eight"][0], parts["eight"][7]
    cap = len(whole["origin"]) + 8
    S, P = fs.SdfGrid, fs.SdfAttrPart

    def refused(pairs, **kw):
        assert raw_merge(fs, pairs, 0, count_only=True, **kw)[0] == -ERR_ARG
        r, outs = raw_merge(fs, pairs, cap, **kw)
        assert r == -ERR_ARG and untouched(outs)

    assert raw_merge(fs, [(a, aa), (b, ba)], cap)[0] > 0                   # the pair merges as it is
    # every refusal of the plain merge
    refused([(a, aa), (b, ba)], n_parts=0)
    assert fs.lib.fluid_sdf_attr_grids_merge(None, None, 2, cap, *[None] * 5) == -ERR_ARG
    refused([(a, aa), (b, ba)], attrs=C.cast(None, C.POINTER(fs.SdfAttrPartC)))            # no records at all
    for missing in range(5):                                               # some output arrays only
        r, outs = raw_merge(fs, [(a, aa), (b, ba)], cap)
        cs = [g._c() for g in (a, b)]
        arr = (fs.SdfGridC * 2)(*[c for c, _ in cs])
        aarr = (fs.SdfAttrPartC * 2)(aa._c(), ba._c())
        outs = [np.full_like(x, FILL) for x in outs]
        ptr = [None if i == missing else x.ctypes.data_as(C.c_void_p) for i, x in enumerate(outs)]
        assert fs.lib.fluid_sdf_attr_grids_merge(arr, aarr, 2, cap, *ptr) == -ERR_ARG and untouched(outs)
    nxt = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    refused([(a, aa), (S(n + 1, b.origin, b.values, b.active, b.background, b.radius, b.half_width), ba)])      # mismatched n
    refused([(a, aa), (S(n, b.origin, np.where(b.active, b.values, np.where(b.values > 0, nxt(b.background), -nxt(b.background))), b.active,
                         nxt(b.background), b.radius, b.half_width), ba)])
    refused([(a, aa), (S(n, b.origin, b.values, b.active, b.background, nxt(b.radius), b.half_width), ba)])
    refused([(a, aa), (S(n, b.origin, b.values, b.active, b.background, b.radius, nxt(b.half_width)), ba)])
    o = b.origin.copy(); o[0, 2] += 4
    refused([(a, aa), (S(n, o, b.values, b.active, b.background, b.radius, b.half_width), ba)])                  # off the 8-grid
    o = b.origin.copy(); o[[0, 1]] = o[[1, 0]]
    refused([(a, aa), (S(n, o, b.values, b.active, b.background, b.radius, b.half_width), ba)])                  # not ascending
    o = b.origin.copy(); o[-1, 0] = (sdf_ref.geometry(n)[1] & ~7) + 8
    refused([(a, aa), (S(n, o, b.values, b.active, b.background, b.radius, b.half_width), ba)])                  # outside the grid's leaves
    v = b.values.copy()
    v[0, np.flatnonzero(~b.active[0])[0]] = 0.75                           # an inactive value that is neither +bg nor -bg
    refused([(a, aa), (S(n, b.origin, v, b.active, b.background, b.radius, b.half_width), ba)])
    # records of another list
    refused([(a, aa), (b, P(ba.id[:-1], ba.velocity[:-1], ba.dist2[:-1]))])
    refused([(a, P(aa.id[:-1], aa.velocity[:-1], aa.dist2[:-1])), (b, ba)])
    # leaves without the three arrays
    bc = ba._c()
    for k in range(3):
        f = [bc.id, bc.velocity, bc.dist2]
        f[k] = None
        refused([(a, aa), (b, ba)], attrs=(fs.SdfAttrPartC * 2)(aa._c(), fs.SdfAttrPartC(bc.n_leaves, *f)))
    # an active voxel with a dist2 that is not finite, or without an id
    leaf, off = np.argwhere(b.active)[len(np.argwhere(b.active)) // 2]
    for bad in (np.inf, np.nan, -np.inf):
        d = ba.dist2.copy(); d[leaf, off] = bad
        refused([(a, aa), (b, P(ba.id, ba.velocity, d))])
    i = ba.id.copy(); i[leaf, off] = NO_ID
    refused([(a, aa), (b, P(i, ba.velocity, ba.dist2))])
    # the part with the smallest dist2 does not hold the smallest active value
    (l, la), (r, ra) = [objects(fs, rec, n, *SETS[1]) for rec in built_records("near", n, *SETS[1], (0, 1))]
    at = {tuple(o): k for k, o in enumerate(r.origin.tolist())}
    done = False
    for k, o in enumerate(map(tuple, l.origin.tolist())):
        if o not in at:
            continue
        both = l.active[k] & r.active[at[o]] & (l.values[k] < r.values[at[o]])
        if both.any():                                                     # a voxel the left particle is closer to: claim otherwise
            d = ra.dist2.copy()
            d[at[o], np.flatnonzero(both)[0]] = 0.0
            refused([(l, la), (r, P(ra.id, ra.velocity, d))])
            refused([(r, P(ra.id, ra.velocity, d)), (l, la)])
            done = True
            break
    assert done
    assert raw_merge(fs, [(l, la), (r, ra)], cap)[0] > 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_attr_merge_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_san_attr_merge"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "vdb_sdf_writer.cpp"),
           os.path.join(ROOT, "tests", "host_san_attr_merge_main.cpp"), "-o", str(exe), "-lz"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host sanitizer run (sdf attribute merge): ok" in r.stdout


FLUID = os.path.join(ROOT, "fluid-simulation_amd", "fluid")


@pytest.mark.parametrize("extra,name", [
    ({"FLUID_BLOCKS": ""}, "FLUID_BLOCKS_MESH"), ({"FLUID_BLOCKS_MESH": "1.5"}, "FLUID_BLOCKS_MESH"),
    ({"FLUID_BLOCKS_MESH": "1.5;2.5"}, "FLUID_BLOCKS_MESH"), ({"FLUID_BLOCKS_MESH": "1.5,2.5,1"}, "FLUID_BLOCKS_MESH"),
    ({"FLUID_BLOCKS_MESH": "a,b"}, "FLUID_BLOCKS_MESH"), ({"FLUID_OUT": ""}, "FLUID_BLOCKS_MESH"), ({"FLUID_STEPS": "0"}, "FLUID_BLOCKS_MESH"),
    ({"FLUID_BLOCKS_MESH": "", "FLUID_BLOCKS_MESH_VEL": "1"}, "FLUID_BLOCKS_MESH_VEL"), ({"FLUID_BLOCKS_MESH_VEL": "x"}, "FLUID_BLOCKS_MESH_VEL"),
    ({"FLUID_BLOCKS_MESH_VEL": "inf"}, "FLUID_BLOCKS_MESH_VEL"), ({"FLUID_BLOCKS_SURFACE": "1.5,2.0"}, "FLUID_BLOCKS_MESH"),
])
def test_driver_refuses_a_block_mesh_it_would_not_write(tmp_path, extra, name):
    """Decided before any handle is created (so this runs without a GPU): return code 1, the variable's name, nothing written."""
    env = dict(os.environ, FLUID_N="16", FLUID_PPC="1", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "simulation"), FLUID_BLOCKS="2x1x1",
               FLUID_BLOCKS_MESH="1.5,2.5")
    for k in ("FLUID_OUT_DENSE", "FLUID_OUT_SURFACE", "FLUID_OUT_MESH", "FLUID_OUT_MESH_VEL", "FLUID_OUT_SMOOTH", "FLUID_BLOCKS_SURFACE",
              "FLUID_BLOCKS_MESH_VEL", "FLUID_SOURCE_EVERY", "FLUID_RAW"):
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and name in r.stderr, (r.returncode, r.stderr[-500:])
    assert not list(tmp_path.rglob("*.ply")) and not list(tmp_path.rglob("*.vdb"))


def test_exports_and_c99_header(tmp_path):
    so = os.path.join(ROOT, "fluid-simulation_amd", "libfluid_hip.so")
    names = ("fluid_dist_sdf_snapshot_attr", "fluid_dist_sdf_wait_attr", "fluid_sdf_attr_grids_merge")
    lib = C.CDLL(so)
    for nm in names:
        assert getattr(lib, nm) is not None
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
        for nm in names:
            assert f" T {nm}\n" in out, nm
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "c99.c"
    src.write_text('#include "fluid_hip.h"\n'
                   "int main(void) { fluid_sdf_attr_part_t p = {0, 0, 0, 0}; (void)p;\n"
                   "  return sizeof(p) > 0 && FLUID_SDF_ATTR_PART_LEAF_BYTES == 10240 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "c99.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
