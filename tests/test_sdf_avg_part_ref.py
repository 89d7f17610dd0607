"""CPU (-m "not gpu"): the reference of the averaged surface's rank records and their merge (tests/sdf_avg_part_ref.py) on its own:
the merge of a split is sdf_avg_ref.averaged() of the union bit for bit, it does not care about the order of the parts, an empty
part is neutral, and the two-particle scene needs the leaves a spheres' list would not hold."""
import numpy as np
import pytest

import sdf_avg_part_ref as part_ref
import sdf_avg_ref
import sdf_ref
from sdf_testlib import u32

PARAMS = [(1.0, 3.0, 1.0, 3.0), (1.5, 2.5, 1.0, 4.0), (1.0, 1.0, 1.0, 4.0), (1.0, 2.0, 0.5, 1.5)]   # (R, w, dx, h)


def same_list(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(u32(got[1]), u32(want[1]))


def one_list(pos, n, R, w, dx, h):
    val, act = sdf_avg_ref.averaged(pos, n, R, w, dx, h)
    return sdf_ref.leaf_list(val, act, sdf_ref.constants(R, w, dx)[3])


@pytest.fixture(scope="module")
def scene():
    pos = sdf_avg_ref.block_and_scattered(24)
    return 24, pos[pos[:, 0] < 0.0], pos[pos[:, 0] >= 0.0]


@pytest.mark.parametrize("R,w,dx,h", PARAMS)
def test_merge_of_a_split_is_the_union(scene, R, w, dx, h):
    n, a, b = scene
    ra, rb = part_ref.record(a, n, R, w, dx, h), part_ref.record(b, n, R, w, dx, h)
    want = one_list(np.vstack([a, b]), n, R, w, dx, h)
    assert len(want[0]) > 0 and len(ra[0]) > 0 and len(rb[0]) > 0
    same_list(part_ref.merge([ra, rb], n, R, w, dx), want)
    same_list(part_ref.merge([rb, ra], n, R, w, dx), want)                      # order-free
    empty = part_ref.record(np.empty((0, 3)), n, R, w, dx, h)
    assert len(empty[0]) == 0
    same_list(part_ref.merge([ra, empty, rb], n, R, w, dx), want)               # an empty part is neutral
    # a record is canonical: +0 and +inf carry no sums, and dist2 is never NaN, negative or -0
    for org, d2, sums in (ra, rb):
        assert not np.isnan(d2).any() and not np.signbit(d2).any()
        assert not sums[np.broadcast_to(((d2 == 0) | np.isinf(d2))[:, None, :], sums.shape)].any()


def test_two_particles_need_the_leaves_beyond_the_band():
    n, (R, w, dx, h), A, B = part_ref.two_particles()
    assert sdf_ref.base_cell(A)[0, 0] == -1 and sdf_ref.base_cell(B)[0, 0] == 2
    ra, rb = part_ref.record(A, n, R, w, dx, h), part_ref.record(B, n, R, w, dx, h)
    want = one_list(np.vstack([A, B]), n, R, w, dx, h)
    same_list(part_ref.merge([ra, rb], n, R, w, dx), want)
    # B's spheres' list: the leaves of its own level set
    sv, sa = sdf_ref.closed(B, n, R, w, dx)
    sph = {tuple(o) for o in sdf_ref.leaf_list(sv, sa, sdf_ref.constants(R, w, dx)[3])[0].tolist()}
    rec = [tuple(o) for o in rb[0].tolist()]
    assert len(rec) == 8 and len(sph) == 4 and sph < set(rec)
    # the merge with B cut down to that list is wrong
    k = np.array([o in sph for o in rec])
    got = part_ref.merge([ra, (rb[0][k], rb[1][k], rb[2][k])], n, R, w, dx)
    dense = lambda l: sdf_ref_dense(l, n, R, w, dx)   # noqa: E731
    wrong = (u32(dense(got)) != u32(dense(want))).sum()
    print(f"two particles: B's record lists {len(rec)} leaves, its spheres' list {len(sph)}; merged by the spheres' rule {wrong} voxels differ")
    assert wrong == 18


def sdf_ref_dense(lst, n, R, w, dx):
    """Values of a leaf list on the padded grid of all leaves, +bg where no leaf is listed."""
    _, _, l0, nl = sdf_ref.geometry(n)
    V = np.full((nl ** 3, 512), sdf_ref.constants(R, w, dx)[3], dtype=np.float32)
    c = (lst[0].astype(np.int64) - l0) // 8
    V[(c[:, 0] * nl + c[:, 1]) * nl + c[:, 2]] = lst[1]
    return V
