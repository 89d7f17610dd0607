"""-m gpu: particle sources and sinks of a block-decomposed run (include/fluid_hip.h, "particle sources and sinks of a decomposed run").

Blocks run as LocalGroup threads of this process on one GPU, as in tests/test_gpu_dist.py.  The references are the numpy
restatements of tests/sources_ref.py and the one-GPU step with the same slots; a decomposed run is never its own reference
(two decomposed runs are compared only where the claim is "this changes nothing")."""
import ctypes as C
import threading

import numpy as np
import pytest

import sources_ref as sr
from conftest import rel_l2
from sources_ref import base_cells, default_solid

pytestmark = pytest.mark.gpu

P_SOURCES = 512
MODES = ["decomposed", "replicated"]


def in_box(bc, lo, hi, grow=0):
    return np.all((bc >= np.asarray(lo) - grow) & (bc <= np.asarray(hi) + grow), axis=1)


def cuts_at(n, dims, x):
    return [[0, x, n] if dims[a] == 2 else [0, n] for a in range(3)]


def apply_slots(sim, slots):
    """The same calls on a FluidSim and on a DistFluidSim (same signatures)."""
    for slot, kw in slots.get("sources", []):
        sim.set_source(slot, **kw)
    for slot, lo, hi in slots.get("sinks", []):
        sim.set_sink(slot, lo, hi)


def run_blocks(fs, dims, n, cuts, mode, pos, vel, body, solid=None, rebalance=None, **kw):
    """body(sim, rank) on one thread per block, after the upload; returns its results by rank and the (closed) sims."""
    fd = fs.load_dist()
    size = dims[0] * dims[1] * dims[2]
    grp = fd.LocalGroup(size)
    sims = [None] * size

    def work(r):
        sim = fd.DistFluidSim(n, dims, cuts, grp.comms[r], dist_solve=mode, **kw)
        sims[r] = sim
        if solid is not None:
            sim.set_solid(solid)
        sim.upload_global(pos, vel)
        if rebalance:
            sim.set_rebalance(*rebalance)
        return body(sim, r)

    try:
        res = grp.run(work)
    finally:
        for s in sims:
            if s is not None:
                s.close()
        grp.close()
    return res, sims


def local(sim):
    p, v, ids = sim.download_local()
    return dict(p=p, v=v, ids=ids, owns=sim.owns(p))


def merged(res):
    ids = np.concatenate([r["ids"] for r in res])
    o = np.argsort(ids, kind="stable")
    return ids[o], np.concatenate([r["p"] for r in res])[o], np.concatenate([r["v"] for r in res])[o]


# ---- 1. ADD across the cuts -------------------------------------------------------------------------------------------------------
def _solid_case(n):
    s = default_solid(n)
    s[19, 3, 5] = 1
    s[21, 2, 4] = 1
    return s


ADD_CASES = [
    # n, dims, cuts, box lo, box hi, solid
    (32, (2, 1, 1), cuts_at(32, (2, 1, 1), 20), (17, 8, 10), (22, 12, 14), None),
    (33, (2, 1, 2), None, (13, 20, 13), (18, 23, 18), None),
    (48, (2, 2, 2), cuts_at(48, (2, 2, 2), 20), (16, 16, 16), (23, 23, 23), None),             # around the corner the eight blocks share
    (32, (2, 1, 1), cuts_at(32, (2, 1, 1), 20), (15, 0, 0), (24, 4, 6), _solid_case),          # reaches outside W, holds solid cells
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,dims,cuts,lo,hi,solid_fn", ADD_CASES)
def test_add_across_the_cuts(fs, mode, n, dims, cuts, lo, hi, solid_fn):
    fd = fs.load_dist()
    cuts = cuts or fd.uniform_cuts(n, dims)
    solid = solid_fn(n) if solid_fn else None
    pos = fs.water_cube_drop(n, 3, seed=0)
    np0, seed, vel = len(pos), 11, (0.25, -1.5, 0.125)

    def body(sim, r):
        sim.set_source(0, lo, hi, 5, mode="add", every=1, vel=vel, seed=seed)
        st = sim.step()
        return dict(local(sim), stats=sim.source_stats(), paths=st["paths"])

    res, _ = run_blocks(fs, dims, n, cuts, mode, pos, None, body, solid=solid)
    want = sr.source_points(n, seed, 0, lo, hi, 5, solid if solid is not None else default_solid(n))
    m = len(want)
    assert m > 0
    if solid_fn:
        assert m < 5 * np.prod(np.asarray(hi) - np.asarray(lo) + 1) * 0.8      # W and the solid cells took their share
    emitting = 0
    for r in res:
        new = r["ids"] >= np0
        assert r["owns"][new].all()                                             # each on the rank that owns its cell
        emitting += bool(new.any())
        assert r["stats"]["emitted_last"] == m and r["stats"]["emitted_total"] == m and r["stats"]["removed_last"] == 0
        assert r["paths"] & P_SOURCES
    assert emitting == len(res)                                                 # the box lies across the cuts: every rank emits
    ids, p, v = merged(res)
    assert np.array_equal(ids[:np0], np.arange(np0))
    assert np.array_equal(ids[np0:], np0 + np.arange(m))
    assert np.array_equal(p[np0:], want)                                        # bit for bit
    assert np.array_equal(v[np0:], np.tile(np.asarray(vel), (m, 1)))


# ---- 1b. a box wholly inside one rank's block ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lo,hi", [((4, 8, 10), (9, 12, 14)), ((6, 9, 11), (6, 9, 11))])
def test_add_inside_one_block(fs, mode, lo, hi):
    """The owner of the whole box places and numbers its points with one scan; the other rank plans the same box, owns none of
    its cells and emits nothing.  Both report the global count."""
    n, dims = 32, (2, 1, 1)
    cuts = cuts_at(n, dims, 20)                                                 # the box lies in x < 20: rank 0's
    pos = fs.water_cube_drop(n, 3, seed=0)
    np0, seed, vel = len(pos), 11, (0.25, -1.5, 0.125)

    def body(sim, r):
        sim.set_source(0, lo, hi, 5, mode="add", every=1, vel=vel, seed=seed)
        st = sim.step()
        return dict(local(sim), stats=sim.source_stats(), paths=st["paths"])

    res, _ = run_blocks(fs, dims, n, cuts, mode, pos, None, body)
    want = sr.source_points(n, seed, 0, lo, hi, 5, default_solid(n))
    m = len(want)
    assert m > 0
    for r in res:
        assert r["stats"]["emitted_last"] == m and r["stats"]["emitted_total"] == m and r["stats"]["removed_last"] == 0
        assert r["paths"] & P_SOURCES
        assert r["owns"][r["ids"] >= np0].all()
    assert (res[0]["ids"] >= np0).sum() == m and not (res[1]["ids"] >= np0).any()   # exactly one rank emits
    ids, p, v = merged(res)
    assert np.array_equal(ids[:np0], np.arange(np0))
    assert np.array_equal(ids[np0:], np0 + np.arange(m))
    assert np.array_equal(p[np0:], want)                                        # bit for bit
    assert np.array_equal(v[np0:], np.tile(np.asarray(vel), (m, 1)))


# ---- 2. FILL with grid velocity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fill_with_grid_velocity(fs, mode):
    fd = fs.load_dist()
    n, dims = 48, (2, 2, 2)
    cuts = [[0, 24, 48], [0, 28, 48], [0, 24, 48]]
    lo, hi = (20, 24, 20), (27, 35, 27)          # across all three cuts; y 24..31 in the cube (index 16..31), 32..35 above it
    pos = fs.water_cube_drop(n, 4, seed=0)
    np0, seed, per_cell = len(pos), 5, 6
    F = fs.FIELD

    def body(sim, r):
        sim.step(); sim.step()
        sim.set_source(0, lo, hi, per_cell, mode="fill", every=1, vel=None, seed=seed)
        st = sim.step()                          # t = 2
        return dict(local(sim), stats=sim.source_stats(), vel=sim.field(F.VEL), paths=st["paths"])

    res, sims = run_blocks(fs, dims, n, cuts, mode, pos, None, body)
    ids, p, v = merged(res)
    assert np.array_equal(ids[:np0], np.arange(np0))
    hist = sr.base_cell_counts(n, lo, hi, p[:np0])          # the old particles where advect left them, over all ranks
    assert hist.max() > 0 and hist.min() == 0
    want = sr.source_points(n, seed, 2, lo, hi, per_cell, default_solid(n), hist)
    m = len(want)
    assert m > 0 and all(r["stats"]["emitted_last"] == m for r in res)
    assert np.array_equal(ids[np0:], np0 + np.arange(m))
    assert np.array_equal(p[np0:], want)
    velgrid = fd.assemble(n, sims, [r["vel"] for r in res])
    want_v = sr.clamped_catmull_rom(n, velgrid, want)
    assert np.abs(want_v).max() > 0
    assert np.array_equal(v[np0:], want_v), np.abs(v[np0:] - want_v).max()
    for r in res:
        assert r["owns"][r["ids"] >= np0].all()


# ---- 3. sink across the cuts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_sink_across_the_cuts(fs, mode):
    fd = fs.load_dist()
    n, dims = 48, (2, 2, 2)
    cuts = fd.uniform_cuts(n, dims)
    lo, hi = (20, 18, 21), (27, 25, 26)          # inside the cube, across the three cut planes at 24
    pos = fs.water_cube_drop(n, 4, seed=0)
    np0 = len(pos)

    def plain(sim, r):
        sim.step()
        return local(sim)

    def with_sink(sim, r):
        sim.set_sink(2, lo, hi)
        st = sim.step()
        a = dict(local(sim), stats=sim.source_stats(), paths=st["paths"])
        sim.clear_sink(2)
        sim.step()
        a["stats2"], a["live2"] = sim.source_stats(), sim.num_live()
        return a

    ref, _ = run_blocks(fs, dims, n, cuts, mode, pos, None, plain)
    res, _ = run_blocks(fs, dims, n, cuts, mode, pos, None, with_sink)
    ids0, p0, v0 = merged(ref)
    ids, p, v = merged(res)
    assert np.array_equal(ids0, np.arange(np0))
    gone = in_box(base_cells(n, p0), lo, hi)
    assert 0 < gone.sum() < np0
    assert not in_box(base_cells(n, p), lo, hi).any()                   # nobody left in the box
    assert np.array_equal(ids, ids0[~gone])                             # exactly the others survive, with their ids ...
    assert np.array_equal(p, p0[~gone]) and np.array_equal(v, v0[~gone])    # ... and their bytes
    for r in res:
        assert r["stats"]["removed_last"] == gone.sum() and r["stats"]["removed_total"] == gone.sum() and r["stats"]["emitted_last"] == 0
        assert r["paths"] & P_SOURCES
        assert r["stats2"]["removed_last"] == 0 and r["stats2"]["removed_total"] == gone.sum()      # a cleared sink removes nothing
    assert sum(r["live2"] for r in res) == np0 - gone.sum()


# ---- 4. whole run against one GPU -------------------------------------------------------------------------------------------------
SCENE_SEED = {48: 0, 32: 0}     # chosen so that the precondition below holds on the one-GPU run
STEPS = 6


def whole_run_slots(n):
    m = int(round(n * 41 / 121))
    a = n // 2 - m // 2
    b = a + m - 1                                   # the cube covers the indices a..b on every axis
    x0, x1 = a + 3, b - 3
    return {"sources": [(0, dict(lo=(x0, b + 2, x0), hi=(x1, b + 3, x1), per_cell=2, mode="add", every=2, vel=None, seed=21)),    # above the cube
                        (3, dict(lo=(x0, b - 1, x0), hi=(x1, b, x1), per_cell=4, mode="fill", every=1, vel=(0.0, -2.0, 0.5), seed=22))],
            "sinks": [(1, (x0, a, x0), (x1, a + 1, x1))]}                                                                           # through its lower part


_single_cache = {}


def single_whole_run(fs, n):
    """The one-GPU run with the slots, once per n.  Before every step the particles also go through a second handle WITHOUT slots:
    its post-advect positions are the ones the sinks and the FILL count see (the second handle starts its solves from 0, which moves
    them by far less than the 1e-6 margin asked of them below)."""
    if n in _single_cache:
        return _single_cache[n]
    pos = fs.water_cube_drop(n, 4, seed=SCENE_SEED[n])
    slots = whole_run_slots(n)
    boxes = [(lo, hi) for _, lo, hi in slots["sinks"]] + [(kw["lo"], kw["hi"]) for _, kw in slots["sources"] if kw["mode"] == "fill"]
    sim, twin = fs.FluidSim(n=n), fs.FluidSim(n=n)
    sim.upload_particles(pos)
    apply_slots(sim, slots)
    st, stats, close_calls = [], [], []
    for i in range(STEPS):
        p, v = sim.download_particles()
        twin.upload_particles(p, v)
        twin.dt = sim.dt
        twin.step()
        pt, _ = twin.download_particles()
        bc = base_cells(n, pt)
        near = np.zeros(len(pt), dtype=bool)
        for lo, hi in boxes:
            near |= in_box(bc, lo, hi, grow=1)
        frac = np.abs(pt[near] - np.floor(pt[near]) - 0.5)
        close_calls.append(int((frac < 1e-6).any(axis=1).sum()))
        st.append(sim.step())
        stats.append(sim.source_stats())
    p, v = sim.download_particles()
    out = dict(np0=len(pos), pos0=pos, st=st, stats=stats, close_calls=close_calls, p=p, v=v, indices=sim.field(fs.FIELD.INDICES))
    sim.close(); twin.close()
    _single_cache[n] = out
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,dims", [(48, (2, 2, 2)), (32, (2, 1, 1)), (32, (1, 1, 1))])
def test_whole_run_against_one_gpu(fs, mode, n, dims):
    fd = fs.load_dist()
    ref = single_whole_run(fs, n)
    # precondition (on the one-GPU run): near the sink and FILL boxes no post-advect coordinate within 1e-6 of a cell face,
    # so that the 1e-9 the two runs may differ by cannot flip a count
    assert ref["close_calls"] == [0] * STEPS, ref["close_calls"]
    assert sum(s["emitted_last"] for s in ref["stats"]) > 0 and sum(s["removed_last"] for s in ref["stats"]) > 0
    slots = whole_run_slots(n)
    F = fs.FIELD

    def body(sim, r):
        apply_slots(sim, slots)
        st, stats = [], []
        for _ in range(STEPS):
            st.append(sim.step())
            stats.append(sim.source_stats())
        return dict(local(sim), st=st, stats=stats, idx=sim.field(F.INDICES))

    res, sims = run_blocks(fs, dims, n, fd.uniform_cuts(n, dims), mode, ref["pos0"], None, body)
    for r in res:
        for k in ("emitted_last", "removed_last", "emitted_total", "removed_total"):
            assert [s[k] for s in r["stats"]] == [s[k] for s in ref["stats"]], (k, [s[k] for s in r["stats"]], [s[k] for s in ref["stats"]])
        assert [s["num_active"] for s in r["st"]] == [s["num_active"] for s in ref["st"]]
    ids, p, v = merged(res)
    assert len(ids) == len(ref["p"]) and len(np.unique(ids)) == len(ids)
    ep, ev = rel_l2(p, ref["p"]), rel_l2(v, ref["v"])
    print(f"whole run {mode} {dims} n={n}: {len(ids)} particles, emitted {[s['emitted_last'] for s in ref['stats']]} removed "
          f"{[s['removed_last'] for s in ref['stats']]} pos {ep:.2e} vel {ev:.2e}")
    assert ep < 1e-9 and ev < 1e-7                       # compare()'s defaults in tests/test_gpu_dist.py
    if mode == "replicated":
        assert ep < 1e-14                                # that file's bound for the replicated mode
    assert np.array_equal(fd.assemble(n, sims, [r["idx"] for r in res]), ref["indices"])


# ---- 5. across a re-balancing -----------------------------------------------------------------------------------------------------
_rebalance_ref = {}


def rebalance_scene(fs):
    n = 64
    pos = fs.water_cube_drop(n, 4, seed=0)
    vel = np.random.default_rng(1).standard_normal(pos.shape) * 0.3
    pos = pos + np.array([7.0, 9.0, -5.0])           # the cube covers the indices x 28..49, y 30..51, z 16..37
    solid = default_solid(n)
    solid[20:30, 2:10, 24:40] = 1
    slots = {"sources": [(0, dict(lo=(30, 54, 20), hi=(37, 55, 27), per_cell=2, mode="add", every=3, vel=(0.0, -1.0, 0.0), seed=31))],
             "sinks": [(0, (36, 30, 24), (41, 32, 29))]}
    return n, pos, vel, solid, slots


@pytest.mark.parametrize("mode", MODES)
def test_across_a_rebalancing(fs, mode):
    """The scene of test_cut_planes_follow_the_water with one source and one sink: the slots, the counters and the ids go with the
    handle into every new window."""
    fd = fs.load_dist()
    n, pos, vel, solid, slots = rebalance_scene(fs)
    steps, dims = 12, (2, 2, 2)
    if "ref" not in _rebalance_ref:
        sim = fs.FluidSim(n=n)
        sim.set_solid(solid)
        sim.upload_particles(pos, vel)
        apply_slots(sim, slots)
        stats = []
        for _ in range(steps):
            sim.step()
            stats.append(sim.source_stats())
        p, v = sim.download_particles()
        _rebalance_ref["ref"] = dict(p=p, v=v, stats=stats, pressure=sim.field(fs.FIELD.PRESSURE))
        sim.close()
    ref = _rebalance_ref["ref"]

    def body(sim, r):
        apply_slots(sim, slots)
        stats = []
        for _ in range(steps):
            sim.step()
            stats.append(sim.source_stats())
        return dict(local(sim), stats=stats, moved=sim.n_rebalanced, pres=sim.field(fs.FIELD.PRESSURE))

    res, sims = run_blocks(fs, dims, n, fd.uniform_cuts(n, dims), mode, pos, vel, body, solid=solid, rebalance=(4, 1.3))
    assert all(r["moved"] >= 1 for r in res), [r["moved"] for r in res]           # the planes moved on every rank
    for r in res:
        assert r["stats"] == res[0]["stats"]                                          # global numbers, the same everywhere
        for k in ("emitted_total", "removed_total"):
            t = [s[k] for s in r["stats"]]
            assert all(b >= a for a, b in zip(t, t[1:])), t                           # ... that survive the new windows
    assert res[0]["stats"] == ref["stats"], (res[0]["stats"], ref["stats"])
    assert ref["stats"][-1]["emitted_total"] > 0 and ref["stats"][-1]["removed_total"] > 0
    ids, p, v = merged(res)
    assert len(ids) == len(ref["p"]) and len(np.unique(ids)) == len(ids)
    ep, ev = rel_l2(p, ref["p"]), rel_l2(v, ref["v"])
    epr = rel_l2(fd.assemble(n, sims, [r["pres"] for r in res]), ref["pressure"])
    print(f"re-balancing with slots {mode}: moved {[r['moved'] for r in res]} pos {ep:.2e} vel {ev:.2e} pressure {epr:.2e}")
    assert ep < 1e-8 and ev < 1e-6 and epr < 1e-7                                     # test_cut_planes_follow_the_water's tolerances


# ---- 6. a rank that cannot grow ---------------------------------------------------------------------------------------------------
def test_a_rank_that_cannot_grow_for_emitted_points_fails_every_rank(fs, monkeypatch):
    """Modelled on test_a_rank_that_cannot_grow_fails_every_rank: almost no spare capacity, an ADD source that gives every rank more
    new points than it has room for, and rank 1 refused the growth.  Every rank must leave that step by itself — rank 1 with its own
    error, the others with FLUID_ERR_PEER — and nobody waits for a peer that has returned (the threads do not wake each other)."""
    monkeypatch.setenv("FLUID_DIST_SLACK", "64")
    monkeypatch.setenv("FLUID_DIST_FAIL_GROW", "1")
    fd = fs.load_dist()
    n, dims = 48, (1, 2, 2)
    pos = fs.water_cube_drop(n, 4, seed=0)
    cuts = fd.uniform_cuts(n, dims)
    grp = fd.LocalGroup(4)
    sims, result = [None] * 4, [None] * 4

    def work(r):
        sim = fd.DistFluidSim(n, dims, cuts, grp.comms[r], dist_solve="decomposed")
        sims[r] = sim
        sim.upload_global(pos)
        sim.set_source(0, (10, 14, 14), (37, 33, 33), 8, mode="add", every=1, vel=(0, 0, 0), seed=1)   # ~ 22 000 points per rank
        for i in range(3):
            try:
                sim.step()
            except Exception as e:  # noqa: BLE001
                result[r] = (i, getattr(e, "code", None), str(e))
                return
        result[r] = (3, 0, "")

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    hung = [r for r, x in enumerate(th) if x.is_alive()]
    if hung:
        fd.lib.fluid_local_group_abort(grp.handle)     # let the stuck threads go before failing
    assert not hung, f"ranks {hung} are still waiting for a peer that has returned"
    print(result)
    assert [res[0] for res in result] == [0] * 4                                     # all of them, in the emitting step
    assert result[1][1] == 2 and "emitted points" in result[1][2] and "refused" in result[1][2]      # FLUID_ERR_HIP where it happened
    assert all(result[r][1] == 5 and "another rank failed" in result[r][2] for r in (0, 2, 3))        # FLUID_ERR_PEER elsewhere
    for s in sims:
        if s is not None:
            s.close()
    grp.close()


# ---- 7. nothing eligible changes nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_nothing_eligible_changes_nothing(fs, mode):
    fd = fs.load_dist()
    n, dims = 32, (2, 2, 1)
    cuts = fd.uniform_cuts(n, dims)
    pos = fs.water_cube_drop(n, 4, seed=0)
    vel = np.random.default_rng(2).standard_normal(pos.shape) * 0.5
    F = fs.FIELD

    def run(with_slots):
        def body(sim, r):
            if with_slots:
                sim.set_source(1, (0, 0, 0), (1, n - 1, n - 1), 4, mode="add", every=1, vel=(1, 0, 0), seed=3)     # wholly outside W
                sim.set_source(2, (n - 2, 3, 3), (n - 1, 9, 9), 4, mode="fill", every=2, vel=None, seed=4)         # too
                sim.set_sink(0, (n - 6, n - 6, n - 6), (n - 3, n - 3, n - 3))                                        # the water never gets there
            st = [sim.step() for _ in range(6)]
            return dict(local(sim), st=st, stats=sim.source_stats(), pres=sim.field(F.PRESSURE), idx=sim.field(F.INDICES))
        return run_blocks(fs, dims, n, cuts, mode, pos, vel, body)[0]

    a, b = run(False), run(True)
    for ra, rb in zip(a, b):
        assert rb["stats"] == dict(emitted_last=0, removed_last=0, emitted_total=0, removed_total=0)
        assert not any(s["paths"] & P_SOURCES for s in rb["st"])
        assert np.array_equal(ra["pres"], rb["pres"]) and np.array_equal(ra["idx"], rb["idx"])
    ia, pa, va = merged(a)
    ib, pb, vb = merged(b)
    assert np.array_equal(ia, ib) and np.array_equal(pa, pb) and np.array_equal(va, vb)


# ---- 8. plain handles -------------------------------------------------------------------------------------------------------------
def test_plain_handles_are_refused(fs):
    sim = fs.FluidSim(n=16)
    h = sim._h
    src = fs.Source()
    src.lo[:] = [4, 4, 4]; src.hi[:] = [6, 6, 6]
    src.per_cell, src.every = 1, 1
    l3, h3 = (C.c_int32 * 3)(4, 4, 4), (C.c_int32 * 3)(6, 6, 6)
    pts = np.zeros((1, 3))
    one = np.zeros(1, dtype=np.uint32)
    x = C.c_int64()
    assert fs.lib.fluid_dist_set_source(h, 0, C.byref(src)) == 3
    assert fs.lib.fluid_dist_set_sink(h, 0, l3, h3) == 3
    assert fs.lib.fluid_dist_get_source_stats(h, C.byref(x), None, None, None) == 3
    assert fs.lib.fluid_dist_add_particles(h, 1, pts.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == 3
    msg = fs.lib.fluid_last_error().decode()
    assert "one-GPU entry points" in msg and "fluid_set_source" in msg
    sim.close()


# ---- fluid_dist_add_particles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_add_particles_with_ids(fs, mode):
    """The caller's points with the caller's ids, on the rank that owns them; vel=None gives clampedCatmullRom over the grid of the
    last step (bit for bit, tests/sources_ref.py); a point of another rank's block is refused and nothing is appended; the next
    source numbers its points after the largest id handed in."""
    fd = fs.load_dist()
    n, dims = 32, (2, 1, 2)
    cuts = fd.uniform_cuts(n, dims)
    pos = fs.water_cube_drop(n, 4, seed=0)
    np0 = len(pos)
    rng = np.random.default_rng(9)
    new = np.concatenate([rng.uniform(-5.5, 5.5, size=(300, 3)), rng.uniform(-14.6, -12.4, size=(40, 3))])    # in the water; at the walls, partly outside W
    newv = rng.standard_normal(new.shape)
    new_ids = (np0 + 1000 + np.arange(len(new))).astype(np.uint32)
    F = fs.FIELD

    def body(sim, r):
        with pytest.raises(fs.FluidError) as e:
            sim.add_particles(np.zeros((0, 3)), None, None)        # no completed step yet
        assert e.value.code == 3
        sim.step(); sim.step()
        vel = sim.field(F.VEL)
        mine = sim.owns(new)
        before = sim.num_live()
        if (~mine).any():
            with pytest.raises(fs.FluidError) as e:
                sim.add_particles(new[:], newv, new_ids)           # some of these belong to other ranks
            assert e.value.code == 1 and sim.num_live() == before
        half = np.arange(len(new)) % 2 == 0
        sim.add_particles(new[mine & half], newv[mine & half], new_ids[mine & half])
        sim.add_particles(new[mine & ~half], None, new_ids[mine & ~half])      # collective: every rank calls it
        a = local(sim)
        sim.set_source(0, (14, 14, 14), (17, 17, 17), 1, mode="add", every=1, vel=(0, 0, 0), seed=1)
        sim.step()
        ids_after = sim.download_local()[2]
        return dict(a, vel=vel, ids_after=ids_after, emitted=sim.source_stats()["emitted_last"])

    res, sims = run_blocks(fs, dims, n, cuts, mode, pos, None, body)
    ids, p, v = merged(res)
    assert np.array_equal(ids, np.concatenate([np.arange(np0), new_ids]))
    assert np.array_equal(p[np0:], new)
    half = np.arange(len(new)) % 2 == 0
    assert np.array_equal(v[np0:][half], newv[half])
    want = sr.clamped_catmull_rom(n, fd.assemble(n, sims, [r["vel"] for r in res]), new[~half])
    assert np.abs(want).max() > 0
    assert np.array_equal(v[np0:][~half], want), np.abs(v[np0:][~half] - want).max()
    for r in res:
        assert r["owns"].all()
    after = np.sort(np.concatenate([r["ids_after"] for r in res]))
    m = res[0]["emitted"]
    assert m > 0 and np.array_equal(after[-m:], int(new_ids.max()) + 1 + np.arange(m))
