"""CPU (-m "not gpu"): the bytes of the .vdb files, pinned.  tests/golden/vdb_bytes.json holds the SHA-256 of every file below with
the header's 36 uuid bytes zeroed, taken from the writers as they were before vdb_format.h stated the format once for both of
them.  FLUID_VDB_ACTIVE_MASK only: zipped bytes depend on the zlib that is installed.  The inputs are the other tests' own
(test_vdb_leaves.fields, test_sdf_host.hand_made), seeded.  `python tests/test_vdb_bytes.py` rewrites the JSON from the library
as built.  The inputs come from numpy's Generator, whose streams a numpy release may change: if every digest fails at once and
the writers have not changed, check out a commit whose writers are known to be good, build it, and regenerate there."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import leaf_ref
import sdf_ref
from test_sdf_host import hand_made
from test_vdb_leaves import fields, leaf_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vdb_bytes.json")
DENSE_N = [8, 31, 130]     # one leaf; partial edge leaves; two 128^3 nodes per axis
SDF_N = [31, 130]
MODE = "active_mask"


def digest(path):
    b = bytearray(open(path, "rb").read())
    b[leaf_ref.UUID] = b"\0" * 36
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def two_fields(n):
    f = fields(n)
    return f["cube"][0], f["random_sparse"][0]


def dense_files(fs, tmp, n):
    """fluid_write_vdb_ex: one file per field; at n = 31 a two-grid file as well."""
    out = {}
    cube, sparse = two_fields(n)
    for name, g in (("cube", cube), ("random_sparse", sparse)):
        fs.write_vdb(tmp / "d.vdb", g, compression=MODE)
        out[f"dense_{n}_{name}"] = digest(tmp / "d.vdb")
    if n == 31:
        fs.write_vdb(tmp / "d2.vdb", [cube, sparse], compression=MODE)
        out["dense_31_two_grids"] = digest(tmp / "d2.vdb")
    return out


def leaf_files(fs, tmp, n):
    """fluid_vdb_append_leaves on two writers in one call; one of them is a two-grid stream that holds a grid already."""
    cube, sparse = two_fields(n)
    w1 = fs.VdbStream(tmp / "l1.vdb", n, 2, compression=MODE)
    w2 = fs.VdbStream(tmp / "l2.vdb", n, 1, compression=MODE)
    w1.append_leaves(leaf_grid(fs, cube))
    w1.append_leaves(leaf_grid(fs, sparse), also=[w2])
    w1.close()
    w2.close()
    return {f"leaves_{n}_stream_of_two": digest(tmp / "l1.vdb"), f"leaves_{n}_step_file": digest(tmp / "l2.vdb")}


def leaf_codes(g):
    """The metadata byte the writer owes each leaf (io/Compression.h:94-100), from the inactive values alone: 0 = none or all
    +bg, 1 = all -bg, 3 = both."""
    bits, bg = g.values.view(np.uint32), np.float32(g.background)
    neg = ((bits == (-bg).view(np.uint32)) & ~g.active).any(axis=1)
    pos = ((bits == bg.view(np.uint32)) & ~g.active).any(axis=1)
    return np.where(~neg, 0, np.where(~pos, 1, 3))


def surface_list(fs, n):
    """test_sdf_host.hand_made and two leaves more, so that at every n the list has what the file format distinguishes: a whole
    leaf of inactive -bg alone (hand_made's all -bg leaf is the last one, which at n = 130 lies mostly outside the grid, where
    voxels are +bg: code 3, not 1), in a root child of its own at n = 130, and active values at the grid's high end."""
    g, val, act = hand_made(fs, n)
    lo, hi, l0, _ = sdf_ref.geometry(n)
    last = hi & ~7

    def box(o):
        return tuple(slice(max(c, lo) - lo, min(c + 7, hi) - lo + 1) for c in o)
    val[box((0, -8, 0))] = -g.background                 # wholly inside the grid at n >= 16
    act[box((0, -8, 0))] = False
    b = box((last, l0 + 8, last))                        # at n = 130 one in-grid voxel deep in x and z
    val[b] = np.random.default_rng(7 * n).uniform(-1, 1, val[b].shape).astype(np.float32)
    act[b] = True
    org, v, a = sdf_ref.leaf_list(val, act, g.background)
    g = fs.SdfGrid(n, org, v, a, g.background, 1.5, 2.5)
    assert g.n_leaves == 6 and set(leaf_codes(g).tolist()) == {0, 1, 3}
    low = (g.origin < lo).any(axis=1)                    # partial leaves at the low end; the high end has one iff hi % 8 != 7
    high = (g.origin + 7 > hi).any(axis=1)
    assert (g.active[low].any(axis=1)).any() and (n != 130 or g.active[high].any(axis=1).any())
    if n == 130:
        assert len({tuple(o) for o in (g.origin // 4096).tolist()}) >= 3 and 1 in leaf_codes(g)[(g.origin[:, 0] >= 0) & (g.origin[:, 1] < 0)]
    return g


def sdf_files(fs, tmp, n):
    """fluid_write_vdb_sdf: a hand-built list with leaves of metadata codes 0, 1 and 3 and partial edge leaves, and an empty list."""
    g = surface_list(fs, n)
    fs.write_vdb_sdf(tmp / "s.vdb", g, MODE)
    empty = fs.SdfGrid(n, np.empty((0, 3)), np.empty((0, 512)), np.empty((0, 512)), 2.5, 1.5, 2.5)
    fs.write_vdb_sdf(tmp / "e.vdb", empty, MODE)
    return {f"sdf_{n}_hand_made": digest(tmp / "s.vdb"), f"sdf_{n}_empty": digest(tmp / "e.vdb")}


CASES = [(dense_files, n) for n in DENSE_N] + [(leaf_files, n) for n in DENSE_N] + [(sdf_files, n) for n in SDF_N]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("make,n", CASES, ids=[f"{m.__name__}_{n}" for m, n in CASES])
def test_bytes_are_the_recorded_ones(fs, tmp_path, golden, make, n):
    got = make(fs, tmp_path, n)
    assert got and all(k in golden for k in got)
    assert got == {k: golden[k] for k in got}


def test_every_recorded_file_is_written(golden):
    """The JSON holds no digest that no case above produces."""
    want = {f"dense_{n}_{f}" for n in DENSE_N for f in ("cube", "random_sparse")} | {"dense_31_two_grids"}
    want |= {f"leaves_{n}_{w}" for n in DENSE_N for w in ("stream_of_two", "step_file")}
    want |= {f"sdf_{n}_{k}" for n in SDF_N for k in ("hand_made", "empty")}
    assert set(golden) == want


if __name__ == "__main__":
    import pathlib
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    lib = entry.load_package()
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        for make_, n_ in CASES:
            rec.update(make_(lib, pathlib.Path(d), n_))
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} digests -> {GOLDEN}")
