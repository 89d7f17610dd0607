"""GPU (-m gpu): the level-set kernels (kernels_sdf_filter.hip, kernels_sdf.hip's track, kernels_sdf_weno.hip, kernels_sdf_flow.hip)
held directly to OpenVDB's own operators, compiled in place over a mock dense grid (oracle/vdb_ref.cpp -> oracle/_ref/libvdb_ref.so;
skipped where that library was not built).  The unfiltered device snapshot — tested against tests/sdf_ref.py elsewhere — is made
dense, the expected list is formed from OpenVDB's passes alone (tests/vdb_cases.py: the pass of the kind, N normalise passes of the
scheme, the trim), and the device's filtered snapshot must have its origins, masks and value bits.  The last test needs no library:
the cloud's positions and OpenVDB's results for it are in tests/golden/vdb_passes.npz."""
import os
import sys

import numpy as np
import pytest

import sdf_flow_ref
import sdf_ref
import vdb_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import vdb_ref  # noqa: E402

pytestmark = pytest.mark.gpu
REF = vdb_ref.ref
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref/libvdb_ref.so not built (needs the reference tree)")
u32 = VC.u32


def is_dense(g, val, act, bg, what):
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    assert g.n_leaves == len(org) and np.array_equal(g.origin, org), (what, g.n_leaves, len(org))
    assert np.array_equal(g.active, a), what
    assert np.array_equal(u32(g.values), u32(v)), (what, int((u32(g.values) != u32(v)).sum()))


def filtered(sim, form, Rad, w):
    kind, W, N, tr, scheme = form
    sim.sdf_set_filter_kind(kind)
    sim.sdf_set_track(N if (N or tr) else None, tr, scheme=VC.SCHEME_NAMES[scheme])
    sim.sdf_snapshot(Rad, w, smooth=(W, 1, 0.0))
    return sim.sdf_wait()


def run_forms(fs, sim, Rad, w, dx, what):
    sim.sdf_snapshot(Rad, w)                               # smooth=None
    plain = sim.sdf_wait()
    assert plain.n_leaves > 0
    val, act = fs.sdf_to_dense(plain)
    bg = plain.background
    assert VC.clean(val) and act.sum() > 100, what
    for form in VC.GPU_FORMS:
        kind, W, N, tr, scheme = form
        ev, ea = VC.flow(REF, kind, val, act, bg, dx, W, 1, N, tr, scheme)
        assert (u32(ev) != u32(val))[act].sum() * 2 > act.sum(), (what, form)       # the filter did something
        is_dense(filtered(sim, form, Rad, w), ev, ea, bg, f"{what} {VC.form_name(form)}")


@needs_ref
@pytest.mark.parametrize("name,n,Rad,w,dx", [("cloud", 16) + VC.GPU_SET,         # two leaves per axis: both halo sides
                                             ("hi", 25, 1.0, 2.0, 0.5),           # a partial last leaf and dx != 1
                                             ("leafcorner", 32) + VC.GPU_SET])    # edge and corner leaves
def test_filtered_snapshot_is_openvdbs(fs, name, n, Rad, w, dx):
    sim = fs.FluidSim(n=n, dx=dx)
    sim.upload_particles(sdf_flow_ref.positions(name, n))
    run_forms(fs, sim, Rad, w, dx, f"{name} {n}")
    sim.close()


@needs_ref
def test_filtered_snapshot_of_the_falling_cube_is_openvdbs(fs):
    Rad, w, dx = VC.GPU_SET
    sim = fs.FluidSim(n=32)
    sim.upload_particles(fs.water_cube_drop(32, 4, seed=0))
    for _ in range(2):
        sim.step()
    run_forms(fs, sim, Rad, w, dx, "water_cube_drop(32, 4) after two steps")
    sim.close()


def test_filtered_snapshot_of_the_cloud_is_the_fixture(fs):
    import make_vdb_golden
    z = np.load(os.path.join(ROOT, "tests", "golden", "vdb_passes.npz"))
    Rad, w, dx = VC.GPU_SET
    sim = fs.FluidSim(n=16, dx=dx)
    sim.upload_particles(z["cloud_pos"])
    bg = sdf_ref.constants(Rad, w, dx)[3]
    for form in VC.FIXTURE_FORMS:
        ev, ea = make_vdb_golden.unpack_cloud(z, form)
        is_dense(filtered(sim, form, Rad, w), ev, ea, bg, VC.form_name(form))
    sim.close()
