"""CPU (-m "not gpu"): fluid_sdf_avg_grids_merge (sdf_avg_host.cpp) on hand-made rank records from tests/sdf_avg_part_ref.py
record(): the merged list against the reference's merge() and against sdf_avg_ref.averaged() of the union, bit for bit; 1, 2 and 3
parts, an empty part, the count-only call, a capacity that is too small, every refusal; the same code under ASan + UBSan as a
stand-alone program whose lists must be the library's; and the driver's refusal of FLUID_BLOCKS_SURFACE_KIND=averaged together
with FLUID_BLOCKS_MESH_VEL."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sdf_avg_part_ref as part_ref
import sdf_avg_ref
import sdf_ref
from sdf_testlib import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid-simulation_amd", "csrc")
ERR_ARG = 1
P = (1.5, 2.5, 1.0, 4.0)                                   # (R, w, dx, h)
P2 = (1.0, 1.0, 1.0, 4.0)                                  # hf > R + w: records list leaves beyond the band


def scene(n):
    """A block of 4^3 cells with 2 points each around the origin and 40 scattered points, some outside the grid."""
    lo, hi, _, _ = sdf_ref.geometry(n)
    rng = np.random.default_rng(100 + n)
    c = np.stack(np.meshgrid(*[np.arange(-2, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.vstack([np.repeat(c, 2, axis=0) + rng.uniform(-0.5, 0.5, (2 * len(c), 3)), rng.uniform(lo - 1.0, hi + 1.0, (40, 3))])


def split(pos, k):
    """k parts: by x at 0, then by y at 0.5 (k = 3); k = 1: the whole."""
    if k == 1:
        return [pos]
    a, b = pos[pos[:, 0] < 0.0], pos[pos[:, 0] >= 0.0]
    return [a, b] if k == 2 else [a, b[b[:, 1] < 0.5], b[b[:, 1] >= 0.5]]


def part_of(fs, rec, n, R, w, dx, h):
    fR, fw, dxf, bg, _, _ = sdf_ref.constants(R, w, dx)
    return fs.SdfAvgPart(n, rec[0], rec[1], rec[2], bg, fR, fw, dxf, np.float32(h))


def same(g, want, what=""):
    assert g.n_leaves == len(want[0]) and np.array_equal(g.origin, want[0]), (what, g.n_leaves, len(want[0]))
    assert np.array_equal(g.active, want[2]), what
    assert np.array_equal(u32(g.values), u32(want[1])), what


@pytest.fixture(scope="module")
def cases():
    """(n, params, k) -> (the parts' positions, their records, the union's list from averaged()), each computed once."""
    out = {}
    for n in (16, 25):
        pos = scene(n)
        for prm in (P, P2):
            R, w, dx, h = prm
            val, act = sdf_avg_ref.averaged(pos, n, R, w, dx, h)
            want = sdf_ref.leaf_list(val, act, sdf_ref.constants(R, w, dx)[3])
            for k in (1, 2, 3):
                pp = split(pos, k)
                out[n, prm, k] = (pp, [part_ref.record(q, n, R, w, dx, h) for q in pp], want)
    return out


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("prm", [P, P2], ids=["band4", "reach_beyond_band"])
@pytest.mark.parametrize("n", [16, 25])
def test_merge_equals_the_reference(fs, cases, n, prm, k):
    R, w, dx, h = prm
    pp, recs, want = cases[n, prm, k]
    assert len(want[0]) > 0 and all(len(q) > 0 for q in pp)
    if n == 25:
        assert want[0].min() < sdf_ref.geometry(n)[0]                           # odd n: the first leaf starts outside the grid
    same_ref = part_ref.merge(recs, n, R, w, dx)
    assert np.array_equal(same_ref[0], want[0]) and np.array_equal(u32(same_ref[1]), u32(want[1]))
    parts = [part_of(fs, r, n, R, w, dx, h) for r in recs]
    g = fs.merge_sdf_avg_grids(parts)
    same(g, want, "merge")
    fR, fw, _, bg, _, _ = sdf_ref.constants(R, w, dx)
    assert g.n == n and (g.background, g.radius, g.half_width) == (bg, fR, fw)
    same(fs.merge_sdf_avg_grids(parts[::-1]), want, "reversed")
    empty = part_of(fs, part_ref.record(np.empty((0, 3)), n, R, w, dx, h), n, R, w, dx, h)
    assert empty.n_leaves == 0
    same(fs.merge_sdf_avg_grids([empty] + parts), want, "an empty part first")
    same(fs.merge_sdf_avg_grids(parts + [empty]), want, "an empty part last")
    assert fs.merge_sdf_avg_grids([empty, empty]).n_leaves == 0
    if k > 1:
        assert sum(p.n_leaves for p in parts) > g.n_leaves                      # some leaf is listed by several parts
    if prm == P2:
        r2 = part_ref.reach2(R, w, dx, h)
        assert any(((p.dist2 >= sdf_ref.constants(R, w, dx)[4]) & (p.dist2 < r2)).any() for p in parts)   # m beyond the band, inside reach


def raw(fs, parts, cap, org, val, act):
    arr = (fs.SdfAvgPartC * max(len(parts), 1))(*parts)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return fs.lib.fluid_sdf_avg_grids_merge(arr, len(parts), cap, p(org), p(val), p(act))


def test_count_capacity_and_refusals(fs, cases):
    n, (R, w, dx, h) = 16, P
    _, recs, want = cases[n, P, 2]
    objs = [part_of(fs, r, n, R, w, dx, h) for r in recs]
    k = len(want[0])

    def cs():
        return [o._c() for o in objs]

    assert raw(fs, cs(), 0, None, None, None) == k                              # the count only: cap_leaves is ignored
    assert raw(fs, cs(), -5, None, None, None) == k
    org, val, act = np.full((k, 3), 77, np.int32), np.full((k, 512), -7.0, np.float32), np.full((k, 8), 99, np.uint64)

    def untouched():
        return (org == 77).all() and (val == -7.0).all() and (act == 99).all()

    assert raw(fs, cs(), k - 1, org, val, act) == -ERR_ARG and untouched()      # too small: nothing written
    assert raw(fs, cs(), k, None, val, act) == -ERR_ARG and raw(fs, cs(), k, org, None, act) == -ERR_ARG
    assert raw(fs, cs(), k, org, val, None) == -ERR_ARG and untouched()
    assert raw(fs, cs(), 0, org, val, act) == -ERR_ARG and raw(fs, [], 0, None, None, None) == -ERR_ARG
    assert fs.lib.fluid_sdf_avg_grids_merge(None, 1, 0, None, None, None) == -ERR_ARG
    for name in ("n", "background", "radius", "half_width", "dx", "influence"):   # scalars that differ as bit patterns
        c = cs()
        v = getattr(c[1], name)
        setattr(c[1], name, v + 1 if name == "n" else float(np.nextafter(np.float32(v), np.float32(100.0))))
        assert raw(fs, c, k, org, val, act) == -ERR_ARG and untouched(), name
    for name, v in (("radius", 0.0), ("half_width", 0.5), ("radius", 2.0), ("dx", 0.0), ("influence", 4.5), ("influence", 0.0)):
        c = cs()                                                                # the same on every part, but not a snapshot's
        for q in c:
            setattr(q, name, v)
        assert raw(fs, c, k, org, val, act) == -ERR_ARG and untouched(), (name, v)

    def broken(change):
        """The merge of the parts with objs[0] replaced by a changed copy."""
        o = objs[0]
        d = dict(origin=o.origin.copy(), dist2=o.dist2.copy(), sums=o.sums.copy())
        change(d)
        b = fs.SdfAvgPart(n, d["origin"], d["dist2"], d["sums"], o.background, o.radius, o.half_width, o.dx, o.influence)
        return raw(fs, [b._c(), objs[1]._c()], k, org, val, act)

    lf, vx = np.argwhere((objs[0].dist2 > 0) & np.isfinite(objs[0].dist2) & (objs[0].sums[:, 0] != 0))[0]
    assert broken(lambda d: None) == k
    same(fs.SdfGrid(n, org, val, np.unpackbits(act.view(np.uint8), axis=1, bitorder="little").astype(bool), 0, 0, 0), want, "raw call")
    org[:], val[:], act[:] = 77, -7.0, 99

    def set_(key, idx, v):
        def f(d):
            d[key][idx] = v
        return f
    bad = {
        "descending": lambda d: d["origin"].__setitem__(slice(None), d["origin"][::-1].copy()),
        "repeated": set_("origin", 1, objs[0].origin[0]),
        "off the 8-grid": set_("origin", (0, 2), objs[0].origin[0, 2] + 4),
        "outside the grid": set_("origin", (-1, 0), 8 * 4096),
        "NaN": set_("dist2", (lf, vx), np.nan),
        "negative": set_("dist2", (lf, vx), -1.0),
        "-0": lambda d: (set_("dist2", (lf, vx), -0.0)(d), set_("sums", (lf, slice(None), vx), 0)(d)),
        "+0 beside sums": set_("dist2", (lf, vx), 0.0),
        "+inf beside sums": set_("dist2", (lf, vx), np.inf),
    }
    for what, change in bad.items():
        assert broken(change) == -ERR_ARG and untouched(), what
    for k_sum in range(4):                                                      # each of the four sums is looked at
        def one(d, k_sum=k_sum):
            d["dist2"][lf, vx] = np.inf
            d["sums"][lf, :, vx] = 0
            d["sums"][lf, k_sum, vx] = 1
        assert broken(one) == -ERR_ARG and untouched(), k_sum
    for field in ("origin", "dist2", "sums"):                                   # leaves without an array
        c = cs()
        setattr(c[0], field, None)
        assert raw(fs, c, k, org, val, act) == -ERR_ARG and untouched(), field
    c = cs()
    c[0].n_leaves = -1
    assert raw(fs, c, k, org, val, act) == -ERR_ARG
    with pytest.raises(fs.FluidError):
        fs.merge_sdf_avg_grids([])


def write_parts(path, parts):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(parts)))
        for p in parts:
            f.write(struct.pack("<ii5f", p.n, p.n_leaves, p.background, p.radius, p.half_width, p.dx, p.influence))
            f.write(p.origin.tobytes() + p.dist2.tobytes() + p.sums.tobytes())


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_merge_under_asan_ubsan(fs, cases, tmp_path):
    exe = tmp_path / "host_san_avg_merge"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "sdf_avg_host.cpp"),
           os.path.join(ROOT, "tests", "host_san_avg_merge_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    sets = []
    for n, prm, k in ((25, P, 3), (16, P2, 2), (25, P2, 1)):
        R, w, dx, h = prm
        parts = [part_of(fs, r, n, R, w, dx, h) for r in cases[n, prm, k][1]]
        if k == 3:
            parts.insert(1, part_of(fs, part_ref.record(np.empty((0, 3)), n, R, w, dx, h), n, R, w, dx, h))   # an empty part between the others
        write_parts(tmp_path / f"san_parts_{len(sets)}.bin", parts)
        sets.append((parts, cases[n, prm, k][2]))
    r = subprocess.run([str(exe), str(tmp_path), str(len(sets))], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host sanitizer run (sdf avg merge): ok" in r.stdout
    for i, (parts, want) in enumerate(sets):                                    # what the sanitized build merged is what the library merges
        blob = (tmp_path / f"san_merged_{i}.bin").read_bytes()
        k = struct.unpack_from("<q", blob)[0]
        g = fs.merge_sdf_avg_grids(parts)
        same(g, want, i)
        words = np.packbits(g.active, axis=1, bitorder="little").view(np.uint64)
        assert k == g.n_leaves and blob[8:] == g.origin.tobytes() + g.values.tobytes() + words.tobytes(), i


def test_driver_refuses_block_velocities_on_the_averaged_surface(tmp_path):
    """FLUID_BLOCKS_SURFACE_KIND=averaged with FLUID_BLOCKS_MESH_VEL, a malformed kind, and a kind with nothing to apply to: refused
    with the reason before any handle is created (no GPU is needed to get there)."""
    from sdf_testlib import FLUID, FLUID_VARS
    base = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k not in ("FLUID_OUT_SURFACE_KIND", "FLUID_BLOCKS_SURFACE_KIND")}
    base.update(FLUID_N="16", FLUID_PPC="1", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "simulation"), FLUID_BLOCKS="2x1x1")
    for extra, word in (({"FLUID_BLOCKS_MESH": "1,3", "FLUID_BLOCKS_MESH_VEL": "1", "FLUID_BLOCKS_SURFACE_KIND": "averaged,3"}, "no closest particle"),
                        ({"FLUID_BLOCKS_SURFACE": "1,3", "FLUID_BLOCKS_SURFACE_KIND": "averaged,4.5"}, "0 < H <= 4"),
                        ({"FLUID_BLOCKS_SURFACE": "1,3", "FLUID_BLOCKS_SURFACE_KIND": "spheres,3"}, "0 < H <= 4"),
                        ({"FLUID_BLOCKS_SURFACE": "1,3", "FLUID_BLOCKS_SURFACE_KIND": "blobs"}, "0 < H <= 4"),
                        ({"FLUID_BLOCKS_SURFACE_KIND": "averaged,3"}, "none of them")):
        r = subprocess.run([FLUID], capture_output=True, text=True, env=dict(base, **extra), cwd=tmp_path, timeout=60)
        assert r.returncode == 1 and "FLUID_BLOCKS_SURFACE_KIND" in r.stderr and word in r.stderr, (extra, r.returncode, r.stderr[-500:])
        assert not list(tmp_path.rglob("*.vdb")), extra
