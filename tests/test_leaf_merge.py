"""fluid_leaf_grids_merge (host only): the leaf lists of the blocks of a decomposed run joined into the list of the whole grid.
The parts are made here in numpy (tests/leaf_ref.py): the leaf list of the dense array with everything outside a block
zeroed — what fluid_dist_output_wait gives on the block's rank.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import leaf_ref
from sdf_testlib import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid-simulation_amd", "csrc")
DIMS = {1: (1, 1, 1), 2: (2, 1, 1), 4: (1, 2, 2), 8: (2, 2, 2)}
ERR_ARG = 1


def cut_of(n):
    """An interior cut at a multiple of 4, near the middle, that falls INSIDE a leaf where the grid has such a place (n > 8)."""
    lo, _, l0, _ = leaf_ref.geometry(n)
    off = l0 - lo
    for c in sorted(range(4, n, 4), key=lambda c: abs(c - n // 2)):
        if (c - off) % 8:
            return c
    return 4 * max(1, n // 8)


def dense_field(n):
    """Sparse by leaf, with a -0.0f and a NaN on either side of the cut plane of every axis (inside one leaf for n > 8)."""
    rng = np.random.default_rng(77 + n)
    lo, _, l0, nl = leaf_ref.geometry(n)
    off = lo - l0
    blocks = rng.random((nl, nl, nl)) < 0.3
    big = np.repeat(np.repeat(np.repeat(blocks, 8, 0), 8, 1), 8, 2)[off:off + n, off:off + n, off:off + n]
    d = np.where((rng.random((n, n, n)) < 0.4) & big, rng.standard_normal((n, n, n)).astype(np.float32), np.float32(0))
    d = np.ascontiguousarray(d, dtype=np.float32)
    c = cut_of(n)
    m = n // 2
    for a in range(3):
        i, j = [m, m, m], [m, m, m]
        i[a], j[a] = c - 1, c
        d[tuple(i)] = -0.0
        d[tuple(j)] = np.nan
    d[1, 1, 1] = -0.0
    d[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1] = np.arange(1, 9, dtype=np.float32).reshape(2, 2, 2)   # the corner eight blocks meet in
    return d


def block_parts(fs, dense, dims):
    n = dense.shape[0]
    c = cut_of(n)
    cuts = [[0, n] if dims[a] == 1 else [0, c, n] for a in range(3)]
    parts = []
    for bx in range(dims[0]):
        for by in range(dims[1]):
            for bz in range(dims[2]):
                z = np.zeros_like(dense)
                sl = tuple(slice(cuts[a][b], cuts[a][b + 1]) for a, b in enumerate((bx, by, bz)))
                z[sl] = dense[sl]
                parts.append(fs.LeafGrid(n, *leaf_ref.leaf_list(z)))
    return parts


@pytest.mark.parametrize("blocks", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [8, 33, 50, 121])
def test_merge_is_the_list_of_the_whole_grid(fs, tmp_path, n, blocks):
    dense = dense_field(n)
    parts = block_parts(fs, dense, DIMS[blocks])
    org, val = leaf_ref.leaf_list(dense)
    if blocks > 1 and n > 8:
        keys = [set(map(tuple, p.origin)) for p in parts]
        shared = max(sum(o in k for k in keys) for o in set().union(*keys))
        assert shared >= 2                                  # a leaf is split by the cut and listed by more than one part
        if blocks == 8:
            assert shared == 8                              # ... the one around the corner all eight blocks meet in, by all of them
    got = fs.merge_leaf_grids(parts)
    assert got.n == n and np.array_equal(got.origin, org)
    assert np.array_equal(u32(got.values), u32(val))        # bit patterns: -0.0f and NaN included
    assert np.array_equal(leaf_ref.scatter(n, got.origin, got.values), u32(dense))
    # the parts in any order, and with an empty part among them
    empty = fs.LeafGrid(n, np.empty((0, 3), np.int32), np.empty((0, 512), np.float32))
    again = fs.merge_leaf_grids(parts[::-1] + [empty])
    assert np.array_equal(again.origin, org) and np.array_equal(u32(again.values), u32(val))
    a, b = tmp_path / "dense.vdb", tmp_path / "merged.vdb"
    fs.write_vdb(a, dense)
    fs.write_vdb_leaves(b, got)
    assert leaf_ref.same_file(a, b)


def raw_merge(fs, parts, cap, org, val):
    arr = (fs.LeafGridC * max(1, len(parts)))(*[p._c() for p in parts])
    return fs.lib.fluid_leaf_grids_merge(arr, len(parts), cap, None if org is None else org.ctypes.data_as(C.c_void_p),
                                         None if val is None else val.ctypes.data_as(C.c_void_p))


def test_count_only_empty_parts_and_refusals(fs):
    n = 33
    dense = dense_field(n)
    parts = block_parts(fs, dense, (2, 2, 2))
    k = len(leaf_ref.leaf_list(dense)[0])
    assert raw_merge(fs, parts, 0, None, None) == k         # the count only
    empty = fs.LeafGrid(n, np.empty((0, 3), np.int32), np.empty((0, 512), np.float32))
    assert raw_merge(fs, [empty, empty, empty], 0, None, None) == 0
    assert fs.merge_leaf_grids([empty, empty]).n_leaves == 0

    org = np.full((k + 2, 3), 0x5A5A5A5A, np.int32)
    val = np.full((k + 2, 512), 7.0, np.float32)

    def refused(ps, cap=k + 2):
        assert raw_merge(fs, ps, cap, org, val) == -ERR_ARG
        assert (org == 0x5A5A5A5A).all() and (val == 7.0).all()            # nothing was written

    assert raw_merge(fs, [empty, empty], k + 2, org, val) == 0
    assert (org == 0x5A5A5A5A).all() and (val == 7.0).all()
    refused(parts, cap=k - 1)                                              # cap_leaves too small
    refused(parts[:-1] + [fs.LeafGrid(n + 1, parts[-1].origin, parts[-1].values)])   # the parts' n differ
    p0 = parts[0]
    assert p0.n_leaves >= 2
    o = p0.origin.copy(); o[1, 2] += 4
    refused([fs.LeafGrid(n, o, p0.values)] + parts[1:])                    # off the 8-grid
    refused([fs.LeafGrid(n, p0.origin[::-1].copy(), p0.values[::-1].copy())] + parts[1:])   # descending
    o = p0.origin.copy(); o[1] = o[0]
    refused([fs.LeafGrid(n, o, p0.values)] + parts[1:])                    # duplicated inside a part
    lo, hi, l0, nl = leaf_ref.geometry(n)
    o = p0.origin.copy(); o[-1, 0] = (hi & ~7) + 8
    refused([fs.LeafGrid(n, o, p0.values)] + parts[1:])                    # beyond the last leaf
    refused(parts + [parts[3]])                                            # two parts hold the same voxels
    # ... and one voxel is enough: +0 in its owner's neighbour becomes a non-zero bit pattern
    keys = [set(map(tuple, p.origin)) for p in parts]
    a, b, both = next((a, b, sorted(keys[a] & keys[b])) for a in range(8) for b in range(a + 1, 8) if keys[a] & keys[b])
    ia = [tuple(x) for x in parts[a].origin].index(both[0])
    ib = [tuple(x) for x in parts[b].origin].index(both[0])
    v = parts[b].values.copy()
    vox = int(np.flatnonzero(u32(parts[a].values[ia]))[0])
    assert u32(v[ib])[vox] == 0
    v[ib, vox] = -0.0
    refused(parts[:b] + [fs.LeafGrid(n, parts[b].origin, v)] + parts[b + 1:])
    with pytest.raises(fs.FluidError) as e:
        fs.merge_leaf_grids(parts + [parts[3]])
    assert e.value.code == ERR_ARG
    # the merge still works afterwards, into the same buffers
    assert raw_merge(fs, parts, k + 2, org, val) == k
    assert np.array_equal(org[:k], leaf_ref.leaf_list(dense)[0]) and (org[k:] == 0x5A5A5A5A).all() and (val[k:] == 7.0).all()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_merge_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_san_merge"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "vdb_writer.cpp"),
           os.path.join(ROOT, "tests", "host_san_merge_main.cpp"), "-o", str(exe), "-lz"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host sanitizer run (merge): ok" in r.stdout
