"""The velocity trails of a decomposed run without a GPU (include/fluid_hip.h, "liquid surface, velocity trails (decomposed runs)"):
the two entry points and their ctypes signatures, what the header says about them, and the driver's refusals around
FLUID_BLOCKS_SURFACE_TRAILS, each before any handle is created."""
import ctypes as C
import os
import subprocess

import pytest

from sdf_testlib import FLUID, FLUID_VARS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fluid_hip.h")
MORE_VARS = ("FLUID_OUT_SURFACE_KIND", "FLUID_BLOCKS_SURFACE_KIND", "FLUID_OUT_SURFACE_TRAILS", "FLUID_BLOCKS_SURFACE_TRAILS")


def test_symbols_and_signatures(fs):
    from fluid_simulation_amd import _lib
    sym = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    P = C.c_void_p
    assert sym["fluid_dist_sdf_snapshot_trails"] == (C.c_int, [P, C.POINTER(fs.SdfParams), C.POINTER(fs.SdfTrails)])
    assert sym["fluid_dist_sdf_trails_stats"] == (C.c_int, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    for name, (res, args) in ((k, sym[k]) for k in ("fluid_dist_sdf_snapshot_trails", "fluid_dist_sdf_trails_stats")):
        f = getattr(fs.lib, name)                                          # the library exports it, and the binding declared it
        assert f.restype is res and list(f.argtypes) == args, name
    assert C.sizeof(fs.SdfTrails) == 32                                    # three doubles, two int32
    # a null handle is refused before anything is touched: no GPU is needed to get there
    assert fs.lib.fluid_dist_sdf_snapshot_trails(None, None, None) == 1 and fs.lib.fluid_dist_sdf_trails_stats(None, None, None) == 1
    for name in ("sdf_snapshot_trails", "sdf_dist_trails_stats"):
        assert callable(getattr(fs.FluidSim, name)) and callable(getattr(fs.load_dist().DistFluidSim, name)), name


def test_header_documents_the_rank_record():
    text = open(HEADER).read()
    assert "int fluid_dist_sdf_snapshot_trails(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_trails_t* t);" in text
    assert "int fluid_dist_sdf_trails_stats(fluid_sim_t* s, int64_t* particles, int64_t* instances);" in text
    assert "liquid surface, velocity trails (decomposed runs)" in text
    sect = text[text.index("---- liquid surface, velocity trails (decomposed runs)"):text.index("int fluid_dist_sdf_trails_stats(")]
    for words in ("fluid_sdf_grids_merge", "Why the merge is exact", "GLOBAL [lo,hi]^3", "FLUID_SDF_LEAF_BYTES", "fluid_dist_sdf_wait",
                  "neither read nor changed", "FLUID_ERR_ARG"):
        assert words in sect, words
    # the one-GPU section no longer lists it as missing
    one = text[text.index("---- liquid surface, velocity trails:"):text.index("typedef struct fluid_sdf_trails {")]
    missing = one[one.index("Not built:"):]
    assert "decomposed" not in missing and "rank record" not in missing
    assert "trails on decomposed runs" not in text


def run(tmp_path, **extra):
    env = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k not in MORE_VARS}
    env.update(FLUID_N="24", FLUID_PPC="1", FLUID_STEPS="1", FLUID_OUT=str(tmp_path / "simulation"), FLUID_BLOCKS="2x1x1")
    env.update(extra)
    return subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)


@pytest.mark.parametrize("extra,word", [
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_TRAILS": "-1"}, "SHUTTER"),
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_TRAILS": "dt,0"}, "SHUTTER"),
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_TRAILS": "dt,1,0.5,33"}, "SHUTTER"),
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_TRAILS": "dt,1,0.5,16,1"}, "SHUTTER"),
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_TRAILS": "fast"}, "SHUTTER"),
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_TRAILS": "dt,1,2"}, "RMIN"),
    ({"FLUID_BLOCKS_SURFACE": "1.5,2", "FLUID_BLOCKS_SURFACE_KIND": "averaged,3", "FLUID_BLOCKS_SURFACE_TRAILS": "dt"}, "exclude"),
    ({"FLUID_BLOCKS_MESH": "1.5,2", "FLUID_BLOCKS_MESH_VEL": "1", "FLUID_BLOCKS_SURFACE_TRAILS": "dt"}, "no attributes"),
    ({"FLUID_BLOCKS_SURFACE_TRAILS": "dt"}, "none of them"),
], ids=["negative", "delta0", "max33", "five_fields", "word", "rmin_above_R", "averaged", "mesh_vel", "no_output"])
def test_driver_refuses(tmp_path, extra, word):
    """Refused with the variable's name and the reason, exit status 1, before any handle is created (no GPU is needed to get there)."""
    r = run(tmp_path, **extra)
    assert r.returncode == 1 and "FLUID_BLOCKS_SURFACE_TRAILS" in r.stderr and word in r.stderr, (extra, r.returncode, r.stderr[-500:])
    assert not list(tmp_path.rglob("*.vdb"))


def test_the_one_gpu_variable_is_still_refused_on_blocks(tmp_path):
    r = run(tmp_path, FLUID_BLOCKS_SURFACE="1.5,2", FLUID_OUT_SURFACE_TRAILS="dt")
    assert r.returncode == 1 and "FLUID_OUT_SURFACE_TRAILS" in r.stderr and "FLUID_BLOCKS" in r.stderr, (r.returncode, r.stderr[-500:])
    assert "FLUID_BLOCKS_SURFACE_TRAILS" in r.stderr                       # it names the block run's variable
    assert not list(tmp_path.rglob("*.vdb"))


def test_the_variable_is_read_with_blocks_only(tmp_path):
    """Without FLUID_BLOCKS it is not read: a malformed value is not refused for its grammar (the run then fails for want of a GPU,
    or runs; either way stderr does not name the variable)."""
    env = {k: v for k, v in os.environ.items() if k not in FLUID_VARS and k not in MORE_VARS}
    env.update(FLUID_N="16", FLUID_PPC="1", FLUID_STEPS="0", FLUID_OUT=str(tmp_path / "simulation"), FLUID_BLOCKS_SURFACE_TRAILS="nonsense")
    r = subprocess.run([FLUID], capture_output=True, text=True, env=env, cwd=tmp_path, timeout=60)
    assert "FLUID_BLOCKS_SURFACE_TRAILS" not in r.stderr, r.stderr[-500:]
