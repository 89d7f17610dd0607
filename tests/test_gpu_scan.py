"""-m gpu: the exclusive prefix sum of the sort and of the unknown numbering (fluid_scan_eval) against numpy.cumsum.

The kernels move 16 bytes per load and store where the addresses allow it and go element by element across the two ends,
so the lengths and start offsets that matter are those around the 2 048-element chunk of a block, the 8 elements of a
thread and the 16-byte boundary (4 ints; 8 flag bytes per thread in the numbering mode), with input and output shifted
alike (the sort: cell_count + c0, cell_start + c0) and apart (no common boundary: the element-wise kernels)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F_SOLID, F_FLUID = 1, 2
CHUNK = 2048
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 255, 256, 257, CHUNK - 9, CHUNK - 8, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 7, CHUNK + 8,
           CHUNK + 9, 2 * CHUNK - 3, 2 * CHUNK, 2 * CHUNK + 5, 5 * CHUNK + 1234, 300_001]
OFFSETS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 13]


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def scan(fs, mode, data, in_off, out_off):
    out = np.full(data.size, -12345, dtype=np.int32)
    total = np.zeros(1, dtype=np.int32)
    rc = fs.lib.fluid_scan_eval(0, mode, data.size, in_off, out_off, P(data), P(out), P(total))
    assert rc == 0, fs.lib.fluid_last_error()
    return out, int(total[0])


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(42)
    ints = rng.integers(0, 9, size=max(LENGTHS), dtype=np.int32)
    ints[rng.random(ints.size) < 0.5] = 0               # cell counts: many empty cells
    flags = rng.choice(np.array([0, F_SOLID, F_FLUID, F_FLUID | (6 << 2), F_FLUID | (3 << 2)], dtype=np.uint8), size=max(LENGTHS))
    ex = np.concatenate([[0], np.cumsum(ints, dtype=np.int64)])
    fl = (flags & F_FLUID) != 0
    exf = np.concatenate([[0], np.cumsum(fl, dtype=np.int64)])
    return ints, ex, flags, fl, exf


@pytest.mark.parametrize("off", OFFSETS)
def test_int_scan_input_and_output_shifted_alike(fs, inputs, off):
    ints, ex, _, _, _ = inputs
    for n in LENGTHS:
        for start in (0, 3):    # another slice of the data, so that a wrong head or tail cannot cancel
            data = np.ascontiguousarray(ints[start:start + n])
            m = data.size
            got, total = scan(fs, 0, data, off, off)
            assert np.array_equal(got, ex[start:start + m] - ex[start]), (n, off, start)
            assert total == ex[start + m] - ex[start]


@pytest.mark.parametrize("offs", [(0, 1), (1, 0), (2, 3), (4, 0), (0, 4), (3, 7), (8, 4), (5, 6)])
def test_int_scan_input_and_output_shifted_apart(fs, inputs, offs):
    ints, ex, _, _, _ = inputs
    for n in LENGTHS:
        got, total = scan(fs, 0, np.ascontiguousarray(ints[:n]), offs[0], offs[1])
        assert np.array_equal(got, ex[:n]), (n, offs)
        assert total == ex[n]


@pytest.mark.parametrize("offs", [(o, o) for o in OFFSETS] + [(0, 1), (1, 0), (4, 0), (0, 4), (8, 4), (3, 7), (16, 8), (12, 4)])
def test_flag_numbering(fs, inputs, offs):
    _, _, flags, fl, exf = inputs
    for n in LENGTHS:
        got, total = scan(fs, 1, np.ascontiguousarray(flags[:n]), offs[0], offs[1])
        want = np.where(fl[:n], exf[:n], -1)
        assert np.array_equal(got, want), (n, offs)
        assert total == exf[n]


def test_all_and_none(fs):
    for n in (CHUNK + 3, 7):
        ones = np.ones(n, dtype=np.int32)
        got, total = scan(fs, 0, ones, 1, 1)
        assert np.array_equal(got, np.arange(n)) and total == n
        got, total = scan(fs, 1, np.zeros(n, dtype=np.uint8), 3, 3)
        assert (got == -1).all() and total == 0
        got, total = scan(fs, 1, np.full(n, F_FLUID, dtype=np.uint8), 5, 5)
        assert np.array_equal(got, np.arange(n)) and total == n
