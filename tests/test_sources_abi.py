"""CPU (-m "not gpu"): the particle sources and sinks at the C ABI — fluid_source_t's layout in C99 against the ctypes Structure,
the new symbols exported by the library, and the numpy restatement of where a source puts its points (tests/sources_ref.py)
against hand-checkable SplitMix64 values."""
import ctypes as C
import os
import subprocess

import numpy as np

import sources_ref as sr
from conftest import ROOT

NEW_SYMBOLS = ("fluid_add_particles", "fluid_set_source", "fluid_set_sink", "fluid_get_source_stats")


def test_source_struct_layout_matches_c(fs, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "fluid_hip.h"
int main(void)
{
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(fluid_source_t), (int)offsetof(fluid_source_t, lo),
           (int)offsetof(fluid_source_t, hi), (int)offsetof(fluid_source_t, per_cell), (int)offsetof(fluid_source_t, mode),
           (int)offsetof(fluid_source_t, every), (int)offsetof(fluid_source_t, vel_mode), (int)offsetof(fluid_source_t, vel),
           (int)offsetof(fluid_source_t, seed), FLUID_MAX_SOURCES, FLUID_MAX_SINKS, FLUID_PATH_SOURCES);
    printf("%d %d %d %d\n", FLUID_SOURCE_ADD, FLUID_SOURCE_FILL, FLUID_SOURCE_VEL_FIXED, FLUID_SOURCE_VEL_GRID);
    return 0;
}
''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    got = [int(x) for x in lines[0].split()]
    S = fs.Source
    want = [C.sizeof(S)] + [getattr(S, f).offset for f in ("lo", "hi", "per_cell", "mode", "every", "vel_mode", "vel", "seed")]
    assert got[:9] == want, (got, want)
    assert got[9:] == [8, 8, 512]
    assert [int(x) for x in lines[1].split()] == [0, 1, 0, 1]


def test_new_symbols_are_exported(fs):
    for name in NEW_SYMBOLS:
        assert hasattr(fs.lib, name), name
    hdr = open(os.path.join(ROOT, "include", "fluid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr


def test_new_entry_points_reject_a_null_handle(fs):
    src = fs.Source()
    assert fs.lib.fluid_add_particles(None, 0, None, None) == 1
    assert fs.lib.fluid_set_source(None, 0, C.byref(src)) == 1
    assert fs.lib.fluid_set_sink(None, 0, None, None) == 1
    assert fs.lib.fluid_get_source_stats(None, None, None, None, None) == 1


def test_splitmix64_known_values():
    # SplitMix64's first three outputs from state 0 (the state advances by the golden gamma): sm(0), sm(g), sm(2g)
    g = 0x9E3779B97F4A7C15
    assert sr.sm64_int(0) == 0xE220A8397B1DCDAF
    assert sr.sm64_int(g) == 0x6E789E6AA1B965F4
    assert sr.sm64_int(2 * g & sr.MASK) == 0x06C45D188009454F
    xs = np.array([0, g, 2 * g & sr.MASK, 12345, sr.MASK], dtype=np.uint64)
    with np.errstate(over="ignore"):
        got = sr.sm64(xs)
    assert [int(v) for v in got] == [sr.sm64_int(int(x)) for x in xs]


def test_source_point_formula_by_hand():
    # seed 7, step 3, cell (x, y, z) = index (5, 6, 7) of n = 16: restated here with Python ints only
    n, seed, t = 16, 7, 3
    idx = np.array([[5, 6, 7]])
    lin = np.array([(5 * n + 6) * n + 7])
    coords = idx - n // 2
    for k in (0, 1, 5):
        key = sr.sm64_int(sr.sm64_int(sr.sm64_int(seed) ^ t) ^ int(lin[0])) ^ k
        want = [float(coords[0, a]) + ((sr.sm64_int((key + a) & sr.MASK) >> 11) * 2.0 ** -53 - 0.5) for a in range(3)]
        p, keep = sr.cell_points(n, seed, t, lin, coords, k)
        assert p[0].tolist() == want
        assert keep[0]


def test_source_points_stay_in_their_cells_and_skip_solid_and_outside_w():
    n = 16
    solid = np.zeros((n, n, n), dtype=np.uint8)
    solid[:2] = solid[-2:] = 1
    solid[:, :2] = solid[:, -2:] = 1
    solid[:, :, :2] = solid[:, :, -2:] = 1
    solid[5, 5, 5] = 1
    pts = sr.source_points(n, 1, 0, (0, 4, 4), (6, 6, 6), 3, solid)
    cells = sr.c_round(pts).astype(np.int64) + n // 2
    assert len(pts) == (6 - 2 + 1) * 3 * 3 * 3 - 3       # x = 2..6 (0, 1 are outside W), minus the solid cell
    assert (cells >= 2).all() and (cells <= n - 3).all()
    assert not solid[cells[:, 0], cells[:, 1], cells[:, 2]].any()
    lin = (cells[:, 0] * n + cells[:, 1]) * n + cells[:, 2]
    assert (np.diff(lin) >= 0).all()                    # pid order: ascending cell
    # FILL: a cell that holds per_cell already gets nothing
    hist = np.zeros((7, 3, 3), dtype=np.int64)
    hist[3, 1, 1] = 3
    hist[4, 1, 1] = 1
    f = sr.source_points(n, 1, 0, (0, 4, 4), (6, 6, 6), 3, solid, hist)
    fc = sr.c_round(f).astype(np.int64) + n // 2
    assert len(f) == len(pts) - 3 - 1
    assert not np.all(fc == [3, 5, 5], axis=1).any()
