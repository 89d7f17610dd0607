"""CPU (-m "not gpu"): the bytes of the three host forms of the level-set filter, pinned.  tests/golden/sdf_filter_bytes.json holds
the SHA-256 of what fluid_sdf_filter, fluid_sdf_filter_tracked and fluid_sdf_filter_grown return and write — the count, origins,
values, masks, `kept`, ids and velocities — taken from sdf_filter_host.cpp as it was before sdf_filter_plan.h stated the schedule
once, and the return code of every refusal that tests/host_san_track_main.cpp and tests/host_san_grow_main.cpp exercise.  The
lists are tests/sdf_ref.py's of three scenes of tests/sdf_grow_ref.py: `cloud` and `faces` at n = 20, `block` at n = 32, where a
leaf has all six neighbours, some neighbours are unlisted, edge leaves are partial, the trim unlists leaves and the dilation adds
them (asserted below).  The cases are the other host tests' own: sdf_filter_ref.FILTERS, sdf_track_ref.TRACKS, sdf_grow_ref.GROWS
and BLOCK_GROWS, the grown ones with and without attributes.  `python tests/test_sdf_filter_bytes.py` rewrites the JSON from the
library as built."""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import attr_ref
import sdf_filter_ref
import sdf_grow_ref as G
import sdf_ref
import sdf_track_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdf_filter_bytes.json")
LISTS = {"cloud": (20, 2.0, 2.0, 1.0), "faces": (20, 2.0, 2.0, 1.0), "block": (32, 3.0, 1.0, 1.0)}      # name: (n, R, w, dx)
FORMS = ["filter", "tracked", "grown"]
ERR_ARG = 1


@functools.lru_cache(maxsize=None)
def lists_of(fs, name):
    """The unfiltered scene as (SdfGrid, SdfAttr, dx)."""
    n, R, w, dx = LISTS[name]
    _, _, val, act, ids, v32, bg = G.base(name, n, R, w, dx)
    fR, fw = sdf_ref.constants(R, w, dx)[:2]
    org, v, a = sdf_ref.leaf_list(val, act, bg)
    li, lv = attr_ref.leaf_attr(ids, v32, org)
    return fs.SdfGrid(n, org, v, a, bg, fR, fw), fs.SdfAttr(li, lv), dx


def digest(count, *arrays):
    h = hashlib.sha256(np.int64(count).tobytes())
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"|{a.dtype.str}{a.shape}|".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def grows_of(name):
    return G.GROWS + (G.BLOCK_GROWS if name == "block" else [])


def digests(fs, name, form):
    g, at, dx = lists_of(fs, name)
    out = {}
    if form == "filter":
        for W, K, off in sdf_filter_ref.FILTERS:
            r = fs.sdf_filter(g, W, K, off)
            out[f"{name}_filter_{W}_{K}_{off}"] = digest(r.n_leaves, r.origin, r.values, r.active)
    elif form == "tracked":
        for W, K, units, N, tr in sdf_track_ref.TRACKS:
            r, kept = fs.sdf_filter_tracked(g, (W, K, units * dx), (N, bool(tr)))
            out[f"{name}_tracked_{W}_{K}_{units}_{N}_{tr}"] = digest(r.n_leaves, r.origin, r.values, r.active, kept)
        r, kept = fs.sdf_filter_tracked(g, (2, 1, 0.5 * dx), None)                # tracking off: fluid_sdf_filter's bytes and every leaf
        out[f"{name}_tracked_off"] = digest(r.n_leaves, r.origin, r.values, r.active, kept)
    else:
        for W, K, units, N in grows_of(name):
            r = fs.sdf_filter_grown(g, (W, K, units * dx), N)
            out[f"{name}_grown_{W}_{K}_{units}_{N}"] = digest(r.n_leaves, r.origin, r.values, r.active)
            r, ra = fs.sdf_filter_grown(g, (W, K, units * dx), N, attr=at)
            out[f"{name}_grown_attr_{W}_{K}_{units}_{N}"] = digest(r.n_leaves, r.origin, r.values, r.active, ra.id, ra.velocity)
    return out


def refusals(fs):
    """name -> return code of every refused call (and of the good calls beside them) of the two sanitizer programs' refusal blocks:
    the tracked function on the cloud's list, the grown one on the `faces` list with its attributes."""
    out = {}
    p = lambda a: None if a is None else C.c_void_p(a if isinstance(a, int) else a.ctypes.data)   # noqa: E731
    filt = lambda f: None if f is None else C.byref(fs.SdfFilter(*f))                             # noqa: E731
    track = lambda t: None if t is None else C.byref(fs.SdfTrack(*t))                             # noqa: E731
    # ---- fluid_sdf_filter_tracked
    g, _, dx = lists_of(fs, "cloud")
    c, words = g._c()
    k0, bg = g.n_leaves, float(g.background)
    org, val, act, kept = np.full((k0, 3), 7, np.int32), np.full((k0, 512), 7, np.float32), np.full((k0, 8), 7, np.uint64), np.full(k0, 7, np.int32)
    ok, tk = (1, 1, 0.0), (3, 1, 0)

    def tcall(f=ok, t=tk, cap=k0, o=org, v=val, a=act, kp=kept, grid=c):
        return int(fs.lib.fluid_sdf_filter_tracked(None if grid is None else C.byref(grid), filt(f), track(t), cap, p(o), p(v), p(a), p(kp)))

    for t in ((-1, 1, 0), (9, 1, 0), (3, 2, 0), (3, 1, 1)):
        out[f"tracked_track_{t}"] = tcall(t=t)
    far = (1, 1, 1.01 * bg)
    out["tracked_offset_beyond_bg"] = tcall(f=far)
    out["tracked_filter_width_5"] = tcall(f=(5, 1, 0.0))
    out["tracked_null_filter"] = tcall(f=None)
    out["tracked_null_grid"] = tcall(grid=None)
    out["tracked_null_values"] = tcall(v=None)
    out["tracked_values_overlap"] = tcall(v=g.values.ctypes.data + 2048)
    out["tracked_origin_is_input"] = tcall(o=g.origin.ctypes.data)
    count = tcall(cap=0, o=None, v=None, a=None, kp=None)
    out["tracked_count_only"] = count
    out["tracked_cap_one_short"] = tcall(cap=count - 1)
    none = fs.SdfGridC(g.n, 0, g.background, g.radius, g.half_width, None, None, None)
    out["tracked_empty_list"] = tcall(cap=0, o=None, v=None, a=None, kp=None, grid=none)
    out["tracked_refusals_wrote"] = int(not ((org == 7).all() and (val == 7).all() and (act == 7).all() and (kept == 7).all()))
    out["tracked_offset_beyond_bg_untracked"] = tcall(f=far, t=None)             # the good calls beside them
    out["tracked_null_track_no_kept"] = tcall(t=None, kp=None)
    # ---- fluid_sdf_filter_grown
    g, at, dx = lists_of(fs, "faces")
    c, words = g._c()
    ac = at._c()
    cap0 = 64
    org, val, act = np.full((cap0, 3), 7, np.int32), np.full((cap0, 512), 7, np.float32), np.full((cap0, 8), 7, np.uint64)
    ids, vel = np.full((cap0, 512), 7, np.uint32), np.full((cap0, 3, 512), 7, np.float32)
    f0, t0 = (1, 0, -3.0 * dx), (3, 1, 0)

    def gcall(a=ac, f=f0, t=t0, cap=cap0, o=org, v=val, m=act, i=ids, ve=vel, grid=c):
        return int(fs.lib.fluid_sdf_filter_grown(C.byref(grid), None if a is None else C.byref(a), filt(f), track(t), cap, p(o), p(v), p(m), p(i), p(ve)))

    for name, t in (("no_pass", (0, 1, 0)), ("no_trim", (3, 0, 0)), ("nine_passes", (9, 1, 0)), ("scheme", (3, 1, 1)), ("null_track", None)):
        out[f"grown_{name}"] = gcall(t=t)
    out["grown_null_filter"] = gcall(f=None)
    four = float(np.float32(4.0) * np.float32(dx))
    out["grown_offset_above_4dx"] = gcall(f=(1, 0, float(np.nextafter(np.float32(four), np.float32(np.inf)))))
    out["grown_null_id"] = gcall(i=None)
    out["grown_null_velocity"] = gcall(ve=None)
    out["grown_outputs_without_attr"] = gcall(a=None)
    out["grown_cap_1"] = gcall(cap=1)
    out["grown_cap_negative"] = gcall(cap=-1)
    out["grown_attr_of_another_list"] = gcall(a=fs.SdfAttrC(g.n_leaves - 1, ac.id, ac.velocity))
    out["grown_attr_without_id"] = gcall(a=fs.SdfAttrC(g.n_leaves, None, ac.velocity))
    out["grown_values_are_input"] = gcall(v=g.values.ctypes.data)
    out["grown_id_is_input"] = gcall(i=at.id.ctypes.data)
    out["grown_refusals_wrote"] = int(not ((org == 7).all() and (val == 7).all() and (act == 7).all() and (ids == 7).all() and (vel == 7).all()))
    out["grown_offset_4dx"] = gcall(f=(1, 0, four))
    none = fs.SdfGridC(g.n, 0, g.background, g.radius, g.half_width, None, None, None)
    out["grown_empty_list"] = gcall(a=None, cap=0, o=None, v=None, m=None, i=None, ve=None, grid=none)
    return out


CASES = [(name, form) for name in LISTS for form in FORMS]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name,form", CASES, ids=[f"{n}_{f}" for n, f in CASES])
def test_bytes_are_the_recorded_ones(fs, golden, name, form):
    got = digests(fs, name, form)
    assert got and all(k in golden["digests"] for k in got)
    assert got == {k: golden["digests"][k] for k in got}


def test_refusals_are_the_recorded_ones(fs, golden):
    got = refusals(fs)
    assert got == golden["refusals"]
    good = {"tracked_count_only", "tracked_empty_list", "tracked_offset_beyond_bg_untracked", "tracked_null_track_no_kept", "grown_offset_4dx",
            "grown_empty_list", "tracked_refusals_wrote", "grown_refusals_wrote"}
    assert all((v >= 0) if k in good else (v == -ERR_ARG) for k, v in got.items())
    assert got["tracked_refusals_wrote"] == 0 and got["grown_refusals_wrote"] == 0


def test_every_recorded_case_is_run(golden):
    """The JSON holds no digest that no case above produces."""
    want = set()
    for name in LISTS:
        want |= {f"{name}_filter_{W}_{K}_{off}" for W, K, off in sdf_filter_ref.FILTERS}
        want |= {f"{name}_tracked_{W}_{K}_{u}_{N}_{tr}" for W, K, u, N, tr in sdf_track_ref.TRACKS} | {f"{name}_tracked_off"}
        want |= {f"{name}_grown{a}_{W}_{K}_{u}_{N}" for W, K, u, N in grows_of(name) for a in ("", "_attr")}
    assert set(golden["digests"]) == want


def test_the_lists_are_not_vacuous(fs):
    """What the sizes were chosen for: a leaf with all six face neighbours listed and leaves with unlisted ones, leaves the grid cuts
    (n = 20), a trim that unlists leaves and a dilation that adds them."""
    six = np.array([[-8, 0, 0], [8, 0, 0], [0, -8, 0], [0, 8, 0], [0, 0, -8], [0, 0, 8]])
    full = partial = shorter = longer = cut = 0
    for name, (n, R, w, dx) in LISTS.items():
        g, at, _ = lists_of(fs, name)
        lo, hi, _, _ = sdf_ref.geometry(n)
        have = {tuple(o) for o in g.origin.tolist()}
        nbs = [sum(tuple(q) in have for q in (o + six).tolist()) for o in g.origin]
        full += 6 in nbs
        partial += any(k < 6 for k in nbs)
        cut += bool(((g.origin < lo) | (g.origin + 7 > hi)).any())
        for W, K, units, N, tr in sdf_track_ref.TRACKS:
            shorter += fs.sdf_filter_tracked(g, (W, K, units * dx), (N, bool(tr)))[0].n_leaves < g.n_leaves
        for W, K, units, N in grows_of(name):
            k = fs.sdf_filter_grown(g, (W, K, units * dx), N).n_leaves
            longer += k > g.n_leaves
            shorter += k < g.n_leaves
    assert full >= 1 and partial >= 1 and cut >= 1 and shorter >= 1 and longer >= 1, (full, partial, cut, shorter, longer)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    lib = entry.load_package()
    rec = {"digests": {}, "refusals": refusals(lib)}
    for name_, form_ in CASES:
        rec["digests"].update(digests(lib, name_, form_))
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec['digests'])} digests, {len(rec['refusals'])} return codes -> {GOLDEN}")
