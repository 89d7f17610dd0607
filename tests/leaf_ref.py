"""The leaf list of a dense grid, in numpy, independent of the library (tests/test_vdb_leaves.py, tests/test_gpu_output.py).

Leaves are OpenVDB's 8^3 blocks with origins at multiples of 8 in index space; array cell a of an axis holds coordinate
lo + a, lo = -(n // 2).  A leaf is listed iff one of its in-grid voxels has a non-zero bit pattern."""
import numpy as np

UUID = slice(21, 57)   # the 36 uuid characters of the header: the only bytes in which two writes of one grid differ


def geometry(n):
    lo = -(n // 2)
    hi = lo + n - 1
    l0 = lo & ~7
    nl = ((hi & ~7) - l0) // 8 + 1
    return lo, hi, l0, nl


def padded(dense):
    """(nl*8)^3 array of bit patterns whose cell (0,0,0) is the first leaf's first voxel; +0 outside the grid."""
    n = dense.shape[0]
    lo, hi, l0, nl = geometry(n)
    off = lo - l0
    p = np.zeros((nl * 8,) * 3, dtype=np.uint32)
    p[off:off + n, off:off + n, off:off + n] = np.ascontiguousarray(dense, dtype=np.float32).view(np.uint32)
    return p, l0, nl


def leaf_blocks(dense):
    """(nl, nl, nl, 512) uint32: every leaf's voxels in ((x&7)*8 + (y&7))*8 + (z&7) order."""
    p, l0, nl = padded(dense)
    return p.reshape(nl, 8, nl, 8, nl, 8).transpose(0, 2, 4, 1, 3, 5).reshape(nl, nl, nl, 512), l0, nl


def listed_mask(dense):
    b, _, _ = leaf_blocks(dense)
    return (b != 0).any(axis=3)


def leaf_list(dense, also=()):
    """(origin (k,3) int32, values (k,512) float32) of the leaves with a non-zero bit pattern, ascending (x, y, z);
    `also`: leaf indices (i, j, k) to name as well, whatever they hold."""
    b, l0, nl = leaf_blocks(dense)
    m = (b != 0).any(axis=3)
    for idx in also:
        m[idx] = True
    ijk = np.argwhere(m)                      # row-major: ascending (x, y, z)
    origin = (l0 + 8 * ijk).astype(np.int32)
    values = b[m].view(np.float32)
    return origin, np.ascontiguousarray(values)


def scatter(n, origin, values):
    """Dense (n,n,n) uint32 bit patterns from a leaf list: the numpy restatement of fluid_leaves_to_dense."""
    lo, hi, l0, nl = geometry(n)
    p = np.zeros((nl * 8,) * 3, dtype=np.uint32)
    v = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).reshape(-1, 8, 8, 8)
    for o, blk in zip(np.asarray(origin).reshape(-1, 3), v):
        a = o - l0
        p[a[0]:a[0] + 8, a[1]:a[1] + 8, a[2]:a[2] + 8] = blk
    off = lo - l0
    return np.ascontiguousarray(p[off:off + n, off:off + n, off:off + n])


def same_file(a, b):
    """Two .vdb files equal byte for byte outside the uuid."""
    x, y = bytearray(open(a, "rb").read()), bytearray(open(b, "rb").read())
    x[UUID] = y[UUID] = b"\0" * 36
    return len(x) == len(y) and x == y
