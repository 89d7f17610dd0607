"""Writes tests/golden/vdb_passes.npz: inputs and the results of OpenVDB's own level-set operators (oracle/_ref/libvdb_ref.so, which
only a machine with the reference tree can build), so that the machines without it still hold the numpy references, the host
library and the kernels to recorded results of OpenVDB's lines.  Run from the repository root after `make -C oracle ref`:
    python tests/golden/make_vdb_golden.py
tests/test_vdb_ref.py::test_library_reproduces_the_fixture shows a stale file.

Stored (float32 unless said; a pass's result is stored at the active voxels only, inactive ones are copies of the input):
  dx, bg                         0.5 and 3 dx
  <field>_val, <field>_act       the rough and the integer field of tests/vdb_cases.py at n = 12, made fit for a leaf list
  <field>_<pass>                 first, hjweno5, laplacian, curvature, median1, median2, box4axis2 (width 4 along axis 2)
  <field>_iter_box1[_<scheme>]   one box iteration of width 1; the same followed by one normalise pass of the scheme
  septuples, sept_*              120 septuples: WENO5 of their first five rows, the biased differences, and the HJWENO5 voxel step of
                                 three septuples that share the middle
  offset_units, _counts, _steps  the offset step lists at dx (units of dx; the lists concatenated)
  box_order                      the axes of the three box passes (int32)
  cloud_pos (float64)            the particles of the "cloud" scene at n = 16, R, w, dx = 2, 2, 1
  cloud_<form>_act, _neg, _val   the filtered level set of the cloud per form of vdb_cases.FIXTURE_FORMS: packed active bits, packed sign
                                 bits of the inactive voxels (-bg or +bg), the active values
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import vdb_cases as VC  # noqa: E402

F = np.float32
N, DX = 12, 0.5
STORED = ("first", "hjweno5", "laplacian", "curvature", "median1", "median2", "box4axis2")
OFFSETS = (0.0, 0.0005, -0.25, 0.5, 0.6, -1.3, 2.0)


def septuples(count, seed):
    """Smooth, rough, clamped and tiny septuples (7, count), the kinds of tests/test_sdf_weno_ref.py."""
    from test_sdf_weno_ref import septuples as s
    return s(count, seed)


def pass_of(ref, name, val, act, bg, dx):
    if name in ("first", "hjweno5"):
        return ref.norm_pass(val, act, bg, dx, VC.FIRST if name == "first" else VC.HJWENO5)
    if name in ("laplacian", "curvature"):
        return getattr(ref, name + "_pass")(val, act, bg, dx)
    if name.startswith("median"):
        return ref.median_pass(val, act, bg, int(name[6:]))
    return ref.box_pass(val, act, bg, int(name[3]), int(name[-1]))


def arrays(ref):
    out = {"dx": F(DX)}
    fields = VC.adversarial(N, DX)
    for field in ("rough", "integer"):
        val, act, bg = fields[field]
        val = VC.as_list_field(val, act, bg)
        out["bg"] = F(bg)
        out[f"{field}_val"], out[f"{field}_act"] = val, act.astype(np.uint8)
        for name in STORED:
            out[f"{field}_{name}"] = pass_of(ref, name, val, act, bg, DX)[act]
        out[f"{field}_iter_box1"] = VC.flow(ref, VC.BOX, val, act, bg, DX, 1, 1)[0][act]
        for scheme in (VC.FIRST, VC.HJWENO5):
            out[f"{field}_iter_box1_{VC.SCHEME_NAMES[scheme]}"] = VC.flow(ref, VC.BOX, val, act, bg, DX, 1, 1, 1, False, scheme)[0][act]
    u = septuples(120, 41)
    out["septuples"] = u
    out["sept_weno5"] = ref.weno5(*u[0:5])
    out["sept_dm"], out["sept_dp"] = ref.axis_diffs(u)
    ux, uy, uz = septuples(120, 42), septuples(120, 43), septuples(120, 44)
    uy[3], uz[3] = ux[3], ux[3]
    out["sept_ux"], out["sept_uy"], out["sept_uz"] = ux, uy, uz
    out["sept_voxel_hjweno5"] = ref.voxel_value(ux, uy, uz, DX, VC.HJWENO5)
    lists = [np.array(ref.offset_steps(F(units) * F(DX), DX), F) for units in OFFSETS]
    out["offset_units"] = np.array(OFFSETS, F)
    out["offset_counts"] = np.array([len(s) for s in lists], np.int32)
    out["offset_steps"] = np.concatenate(lists).astype(F)
    out["box_order"] = np.array(ref.box_order()[0], np.int32)
    import sdf_flow_ref
    R, w, dx = VC.GPU_SET
    out["cloud_pos"] = np.array(sdf_flow_ref.positions("cloud", 16), np.float64)
    val, act, bg = VC.scene_field("cloud", 16, R, w, dx)
    for form in VC.FIXTURE_FORMS:
        kind, W, Np, tr, scheme = form
        v, a = VC.flow(ref, kind, val, act, bg, dx, W, 1, Np, tr, scheme)
        assert (np.abs(v[~a]) == F(bg)).all()
        key = "cloud_" + VC.form_name(form)
        out[key + "_act"], out[key + "_neg"], out[key + "_val"] = np.packbits(a), np.packbits(~a & (v < 0)), v[a]
    return out


def unpack_cloud(z, form, n=16):
    """(val, act) dense of a stored form."""
    key = "cloud_" + VC.form_name(form)
    act = np.unpackbits(z[key + "_act"])[:n ** 3].astype(bool).reshape(n, n, n)
    neg = np.unpackbits(z[key + "_neg"])[:n ** 3].astype(bool).reshape(n, n, n)
    R, w, dx = VC.GPU_SET
    bg = F(F(dx) * F(w))
    val = np.where(neg, -bg, bg).astype(F)
    val[act] = z[key + "_val"]
    return val, act


if __name__ == "__main__":
    from oracle import vdb_ref
    assert vdb_ref.ref is not None, "build oracle/_ref/libvdb_ref.so first (make -C oracle ref)"
    path = os.path.join(HERE, "vdb_passes.npz")
    np.savez_compressed(path, **arrays(vdb_ref.ref))
    print(path, os.path.getsize(path), "bytes")
