#!/usr/bin/env python3
"""Host cost and bytes of the .vdb writers and the leaf-list merges, two builds side by side (no GPU):
    python tools/vdb_host_cost.py --parent A.so --new B.so [bytes] [time] [--reps 9] [--out DIR]

A.so / B.so: csrc/vdb_writer.cpp and csrc/vdb_sdf_writer.cpp of two commits, each built alone with the Makefile's flags,
    g++ -O2 -std=c++17 -fPIC -shared -Iinclude fluid-simulation_amd/csrc/vdb_writer.cpp fluid-simulation_amd/csrc/vdb_sdf_writer.cpp -o A.so -lz
and loaded into this one process through ctypes.
bytes   ZIP | ACTIVE_MASK and ACTIVE_MASK files of both builds at n = 8, 31, 121, 130, 256 (dense fields of tests/test_vdb_leaves.py,
        random leaves at 121 and 256; a two-grid file; one fluid_vdb_append_leaves call on two writers; a surface list with every
        metadata code and an empty one), compared with cmp after zeroing the header's 36 uuid bytes.
time    one fluid_vdb_append_leaves call on two writers, one fluid_write_vdb, one fluid_write_vdb_sdf at n = 121 and 256 with
        15 % of the leaves listed, zip on, and the three merges on four parts at n = 121 (count-only call + writing call, the
        output arrays allocated inside the timed span); the builds alternated, the order swapped every repeat, one warm-up.
        Prints the table of profiles/output/NOTES.md: the new median may exceed the parent's by the parent's min-to-max spread.
        Then the density merge alone, 400 alternated repeats into preallocated arrays.
Files go to --out (default: a temporary directory; a memory file system keeps the disk out of the numbers)."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import leaf_ref   # noqa: E402
import sdf_ref    # noqa: E402
from test_vdb_leaves import fields   # noqa: E402

OUT = None    # set in main
LIBS = {}     # "parent", "new" -> CDLL
P = C.c_void_p


class LeafGridC(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_leaves", C.c_int32), ("origin", P), ("values", P)]


class SdfGridC(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_leaves", C.c_int32), ("background", C.c_float), ("radius", C.c_float),
                ("half_width", C.c_float), ("origin", P), ("values", P), ("active", P)]


class AttrPartC(C.Structure):
    _fields_ = [("n_leaves", C.c_int32), ("id", P), ("velocity", P), ("dist2", P)]


def load(path):
    lib = C.CDLL(path)
    lib.fluid_leaf_grids_merge.restype = C.c_int64
    lib.fluid_sdf_grids_merge.restype = C.c_int64
    lib.fluid_sdf_attr_grids_merge.restype = C.c_int64
    lib.fluid_leaf_grids_merge.argtypes = [P, C.c_int32, C.c_int64, P, P]
    lib.fluid_sdf_grids_merge.argtypes = [P, C.c_int32, C.c_int64, P, P, P]
    lib.fluid_sdf_attr_grids_merge.argtypes = [P, P, C.c_int32, C.c_int64, P, P, P, P, P]
    lib.fluid_vdb_open.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, P]
    lib.fluid_vdb_append.argtypes = [P, P]
    lib.fluid_vdb_close.argtypes = [P]
    lib.fluid_vdb_append_leaves.argtypes = [P, C.c_int32, P]
    lib.fluid_write_vdb_ex.argtypes = [C.c_char_p, C.c_int32, C.c_int32, P, C.c_int32]
    lib.fluid_write_vdb_sdf.argtypes = [C.c_char_p, P, C.c_int32]
    return lib


def ptr(a):
    return a.ctypes.data_as(P)


def sparse_field(n, frac=0.15, seed=7):
    lo, hi, l0, nl = leaf_ref.geometry(n)
    rng = np.random.default_rng(seed + n)
    blocks = rng.random((nl, nl, nl)) < frac
    off = lo - l0
    big = np.repeat(np.repeat(np.repeat(blocks, 8, 0), 8, 1), 8, 2)[off:off + n, off:off + n, off:off + n]
    r = np.where((rng.random((n, n, n)) < 0.3) & big, rng.standard_normal((n, n, n)).astype(np.float32), np.float32(0))
    return np.ascontiguousarray(r, dtype=np.float32)


def sdf_list(n, frac=0.15, seed=11, bg=np.float32(2.5)):
    """(origin, values, active words): random leaves; per leaf active where k > 0.4, the rest -bg / +bg (codes 0, 1, 3 all occur)."""
    lo, hi, l0, nl = sdf_ref.geometry(n)
    rng = np.random.default_rng(seed + n)
    k = np.flatnonzero(rng.random(nl ** 3) < frac)
    org = (np.stack([k // (nl * nl), (k // nl) % nl, k % nl], axis=1) * 8 + l0).astype(np.int32)
    m = len(k)
    u = rng.random((m, 512))
    kind = rng.integers(0, 3, m)[:, None]          # 0: inactive +bg only, 1: -bg only, 2: both
    act = u > 0.4
    val = rng.uniform(-bg, bg, (m, 512)).astype(np.float32)
    neg = np.where(kind == 0, False, np.where(kind == 1, True, u <= 0.2))
    val = np.where(act, val, np.where(neg, -bg, bg)).astype(np.float32)
    words = np.ascontiguousarray(np.packbits(act, axis=1, bitorder="little").view("<u8").reshape(-1, 8))
    return np.ascontiguousarray(org), np.ascontiguousarray(val), words


def leafgrid(n, dense):
    org, val = leaf_ref.leaf_list(dense)
    org, val = np.ascontiguousarray(org), np.ascontiguousarray(val)
    return LeafGridC(n, len(org), org.ctypes.data, val.ctypes.data), (org, val)


def sdfgrid(n, lst, bg=2.5):
    org, val, words = lst
    return SdfGridC(n, len(org), bg, 1.5, 2.5, org.ctypes.data if len(org) else None, val.ctypes.data if len(org) else None,
                    words.ctypes.data if len(org) else None), lst


# ---- operations: each returns the files it wrote -------------------------------------------------------------------------------
def op_dense(lib, tag, n, grids, comp):
    path = f"{OUT}/{tag}_dense.vdb"
    arr = (P * len(grids))(*[g.ctypes.data for g in grids])
    assert lib.fluid_write_vdb_ex(path.encode(), n, len(grids), arr, comp) == 0
    return [path]


def op_leaves(lib, tag, n, g_first, g_both, comp):
    """two writers, one a two-grid stream"""
    p1, p2 = f"{OUT}/{tag}_l1.vdb", f"{OUT}/{tag}_l2.vdb"
    w1, w2 = P(), P()
    assert lib.fluid_vdb_open(p1.encode(), n, 2, comp, C.byref(w1)) == 0
    assert lib.fluid_vdb_open(p2.encode(), n, 1, comp, C.byref(w2)) == 0
    one = (P * 1)(w1.value)
    assert lib.fluid_vdb_append_leaves(one, 1, C.byref(g_first)) == 0
    two = (P * 2)(w1.value, w2.value)
    t0 = time.perf_counter()
    assert lib.fluid_vdb_append_leaves(two, 2, C.byref(g_both)) == 0
    dt = time.perf_counter() - t0
    assert lib.fluid_vdb_close(w1) == 0 and lib.fluid_vdb_close(w2) == 0
    return [p1, p2], dt


def op_sdf(lib, tag, g, comp):
    path = f"{OUT}/{tag}_sdf.vdb"
    assert lib.fluid_write_vdb_sdf(path.encode(), C.byref(g), comp) == 0
    return [path]


def masked(path):
    b = bytearray(open(path, "rb").read())
    b[21:57] = b"\0" * 36
    open(path + ".m", "wb").write(b)
    return path + ".m"


def compare_bytes():
    n_files = 0
    for comp in (3, 2):
        for n in (8, 31, 121, 130, 256):
            if n in (8, 31, 130):
                f = fields(n)
                cube, sp = f["cube"][0], f["random_sparse"][0]
            else:
                cube, sp = sparse_field(n, 0.05, 3), sparse_field(n)
            g1, k1 = leafgrid(n, cube)
            g2, k2 = leafgrid(n, sp)
            sg, k3 = sdfgrid(n, sdf_list(n))
            se, k4 = sdfgrid(n, (np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 8), np.uint64)))
            files = {}
            for name, lib in LIBS.items():
                t = f"{name}_{n}_{comp}"
                fl = op_dense(lib, t + "_cube", n, [cube], comp) + op_dense(lib, t + "_sp", n, [sp], comp)
                if n <= 130:
                    fl += op_dense(lib, t + "_two", n, [cube, sp], comp)
                fl += op_leaves(lib, t, n, g1, g2, comp)[0]
                fl += op_sdf(lib, t + "_rand", sg, comp) + op_sdf(lib, t + "_empty", se, comp)
                files[name] = fl
            for a, b in zip(files["parent"], files["new"]):
                r = subprocess.run(["cmp", masked(a), masked(b)], capture_output=True, text=True)
                assert r.returncode == 0, (a, b, r.stdout)
                n_files += 1
                for p in (a, b, a + ".m", b + ".m"):
                    os.remove(p)
            print(f"comp={comp} n={n}: {len(files['new'])} files identical (sdf leaves {sg.n_leaves})", flush=True)
    print(f"cmp: {n_files} file pairs identical")


def merge_parts(n=121):
    """four parts: density split by quadrants of (x, y); surface lists as overlapping random subsets with their own values"""
    dense = sparse_field(n, 0.3, 5)
    h = n // 2
    leaf_parts, keep = [], []
    for qx in (0, 1):
        for qy in (0, 1):
            d = np.zeros_like(dense)
            sx = slice(0, h) if qx == 0 else slice(h, n)
            sy = slice(0, h) if qy == 0 else slice(h, n)
            d[sx, sy, :] = dense[sx, sy, :]
            g, k = leafgrid(n, d)
            leaf_parts.append(g); keep.append(k)
    org, val, words = sdf_list(n, 0.3, 13)
    rng = np.random.default_rng(99)
    sdf_parts, attr_parts = [], []
    for p in range(4):
        sel = np.flatnonzero(rng.random(len(org)) < 0.6)
        o = np.ascontiguousarray(org[sel])
        act = rng.random((len(sel), 512)) > 0.4
        d2 = rng.random((len(sel), 512)).astype(np.float32)
        v = np.where(act, d2, np.float32(2.5)).astype(np.float32)     # active value = dist2: the closest part holds the smallest value
        w = np.ascontiguousarray(np.packbits(act, axis=1, bitorder="little").view("<u8").reshape(-1, 8))
        ids = rng.integers(0, 2 ** 31, (len(sel), 512)).astype(np.uint32)
        vel = rng.standard_normal((len(sel), 1536)).astype(np.float32)
        v = np.ascontiguousarray(v)
        sdf_parts.append(SdfGridC(n, len(sel), 2.5, 1.5, 2.5, o.ctypes.data, v.ctypes.data, w.ctypes.data))
        attr_parts.append(AttrPartC(len(sel), ids.ctypes.data, vel.ctypes.data, d2.ctypes.data))
        keep.append((o, v, w, ids, vel, d2))
    return (LeafGridC * 4)(*leaf_parts), (SdfGridC * 4)(*sdf_parts), (AttrPartC * 4)(*attr_parts), keep


def run_merges(lib, parts):
    lp, sp, ap, _ = parts
    out = {}
    t0 = time.perf_counter()
    k = lib.fluid_leaf_grids_merge(lp, 4, 0, None, None)
    assert k > 0
    o, v = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32)
    assert lib.fluid_leaf_grids_merge(lp, 4, k, ptr(o), ptr(v)) == k
    out["leaf_grids_merge"] = (time.perf_counter() - t0, [o, v])
    t0 = time.perf_counter()
    k = lib.fluid_sdf_grids_merge(sp, 4, 0, None, None, None)
    assert k > 0
    o, v, w = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.empty((k, 8), np.uint64)
    assert lib.fluid_sdf_grids_merge(sp, 4, k, ptr(o), ptr(v), ptr(w)) == k
    out["sdf_grids_merge"] = (time.perf_counter() - t0, [o, v, w])
    t0 = time.perf_counter()
    k = lib.fluid_sdf_attr_grids_merge(sp, ap, 4, 0, None, None, None, None, None)
    assert k > 0, k
    o, v, w = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.empty((k, 8), np.uint64)
    i, ve = np.empty((k, 512), np.uint32), np.empty((k, 1536), np.float32)
    assert lib.fluid_sdf_attr_grids_merge(sp, ap, 4, k, ptr(o), ptr(v), ptr(w), ptr(i), ptr(ve)) == k
    out["sdf_attr_grids_merge"] = (time.perf_counter() - t0, [o, v, w, i, ve])
    return out


def timings(reps=9):
    t = {}

    def add(key, name, dt):
        t.setdefault(key, {"parent": [], "new": []})[name].append(dt * 1e3)
    for n in (121, 256):
        sp = sparse_field(n)
        first = sparse_field(n, 0.05, 3)
        g1, k1 = leafgrid(n, first)
        g2, k2 = leafgrid(n, sp)
        sg, k3 = sdfgrid(n, sdf_list(n))
        print(f"n={n}: density leaves listed {g2.n_leaves} of {leaf_ref.geometry(n)[3] ** 3}, surface leaves {sg.n_leaves}", flush=True)
        for r in range(reps + 1):
            for name, lib in (list(LIBS.items())[::-1] if r % 2 else list(LIBS.items())):
                tag = f"t_{name}"
                fl, dt = op_leaves(lib, tag, n, g1, g2, 3)
                t0 = time.perf_counter(); fl += op_dense(lib, tag, n, [sp], 3); d2 = time.perf_counter() - t0
                t0 = time.perf_counter(); fl += op_sdf(lib, tag, sg, 3); d3 = time.perf_counter() - t0
                for p in fl:
                    os.remove(p)
                if r == 0:
                    continue      # warm-up
                add(f"fluid_vdb_append_leaves, 2 writers, n={n}", name, dt)
                add(f"fluid_write_vdb, n={n}", name, d2)
                add(f"fluid_write_vdb_sdf, n={n}", name, d3)
    parts = merge_parts()
    ref = None
    for r in range(reps + 1):
        for name, lib in (list(LIBS.items())[::-1] if r % 2 else list(LIBS.items())):
            out = run_merges(lib, parts)
            if ref is None:
                ref = out
            for k, (dt, arrs) in out.items():
                assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(arrs, ref[k][1])), k
                if r:
                    add(f"fluid_{k}, 4 parts, n=121 (count + write)", name, dt)
    print("| call | parent median ms | parent min..max ms | new median ms | new min..max ms | new - parent | allowed (parent spread) | ok |")
    print("|---|---|---|---|---|---|---|---|")
    for k, v in t.items():
        p, q = v["parent"], v["new"]
        pm, qm = statistics.median(p), statistics.median(q)
        spread = max(p) - min(p)
        print(f"| {k} | {pm:.2f} | {min(p):.2f}..{max(p):.2f} | {qm:.2f} | {min(q):.2f}..{max(q):.2f} | {qm - pm:+.2f} | {spread:.2f} | {'yes' if qm - pm <= spread else 'NO'} |")
    print(f"merged outputs of parent and new identical in every repeat; {reps} repeats each, alternated, after one warm-up")


def density_merge_alone(reps=400):
    lp = merge_parts()
    k = LIBS["new"].fluid_leaf_grids_merge(lp[0], 4, 0, None, None)
    o, v = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32)
    res = {"parent": [], "new": []}
    for r in range(reps):
        for name in (("parent", "new") if r % 2 else ("new", "parent")):
            lib = LIBS[name]
            t0 = time.perf_counter()
            lib.fluid_leaf_grids_merge(lp[0], 4, 0, None, None)
            t1 = time.perf_counter()
            lib.fluid_leaf_grids_merge(lp[0], 4, k, ptr(o), ptr(v))
            res[name].append((t1 - t0, time.perf_counter() - t1))
    for name, x in res.items():
        print(f"fluid_leaf_grids_merge alone, {k} merged leaves, {name}: count-only {1e3 * statistics.median(a for a, _ in x):.3f} ms, "
              f"writing call {1e3 * statistics.median(b for _, b in x):.3f} ms (medians of {reps})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", help="bytes, time (default: both)")
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.what = a.what or ["bytes", "time"]
    assert set(a.what) <= {"bytes", "time"}, a.what
    LIBS.update(parent=load(a.parent), new=load(a.new))
    with tempfile.TemporaryDirectory(dir=a.out) as OUT:
        if "bytes" in a.what:
            compare_bytes()
        if "time" in a.what:
            timings(a.reps)
            density_merge_alone()
