"""CPU (-m "not gpu"): the particle sources and sinks of a decomposed run at the C ABI — the four fluid_dist_* symbols exported
and declared, a NULL handle rejected, and the header (with its new block) still a C99 header."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NEW_SYMBOLS = ("fluid_dist_set_source", "fluid_dist_set_sink", "fluid_dist_get_source_stats", "fluid_dist_add_particles")


def test_new_symbols_are_exported_and_declared(fs):
    hdr = open(os.path.join(ROOT, "include", "fluid_hip.h")).read()
    one_gpu = hdr.index("int fluid_get_source_stats(")
    for name in NEW_SYMBOLS:
        assert hasattr(fs.lib, name), name
        assert hdr.index("int " + name + "(") > one_gpu, name      # the new block follows the one-GPU block
    fd = fs.load_dist()
    for m in ("set_source", "clear_source", "set_sink", "clear_sink", "source_stats", "add_particles"):
        assert m in vars(fd.DistFluidSim), m                        # the decomposed handle's own, not FluidSim's


def test_new_entry_points_reject_a_null_handle(fs):
    src = fs.Source()
    l3 = (C.c_int32 * 3)(2, 2, 2)
    assert fs.lib.fluid_dist_set_source(None, 0, C.byref(src)) == 1
    assert fs.lib.fluid_dist_set_sink(None, 0, l3, l3) == 1
    assert fs.lib.fluid_dist_get_source_stats(None, None, None, None, None) == 1
    assert fs.lib.fluid_dist_add_particles(None, 0, None, None, None) == 1
    assert "null handle" in fs.lib.fluid_last_error().decode()


def test_header_still_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text(r'''
#include "fluid_hip.h"
typedef int (*set_source_t)(fluid_sim_t*, int32_t, const fluid_source_t*);
typedef int (*set_sink_t)(fluid_sim_t*, int32_t, const int32_t[3], const int32_t[3]);
typedef int (*stats_t)(fluid_sim_t*, int64_t*, int64_t*, int64_t*, int64_t*);
typedef int (*add_t)(fluid_sim_t*, int64_t, const double*, const double*, const uint32_t*);
int main(void)
{
    set_source_t a = fluid_dist_set_source;
    set_sink_t b = fluid_dist_set_sink;
    stats_t c = fluid_dist_get_source_stats;
    add_t d = fluid_dist_add_particles;
    return (a && b && c && d) ? 0 : 1;
}
''')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "use.o")])
