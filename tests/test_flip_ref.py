"""CPU (-m "not gpu"): pins tests/flip_ref.py, the numpy restatement of FLIPadvect that tests/test_gpu_g2p.py holds the
device to, bit for bit.

 * it equals Oracle.flip_advect to the last bit (positions, velocities, max_speed, dt) on the oracle's own state after a
   pressure pass, the obstacle scene, blends 1, 0.95 and 0, half-integer ties, the shell, off-grid particles, and fast
   particles aimed at walls and obstacles from all six directions at negative coordinates;
 * and on adversarial fields loaded with Oracle.set_field (independent random faces everywhere, 1e3 outside W);
 * the comparison discriminates: one face inside W changes exactly the particles that weigh its cell, one outside W changes
   nothing, and a restatement with W moved by one or floor in place of truncation no longer matches.
"""
import numpy as np
import pytest

import flip_ref as fr
import sources_ref as sr


def _run_oracle(orc):
    """Oracle.flip_advect on its current state: (inputs, outputs) with inputs = (vel, velBefore, pos, pvel)."""
    pos, pvel = orc.particles()
    ins = (orc.field(2), orc.field(3), pos, pvel)
    orc.flip_advect()
    po, vo = orc.particles()
    st = orc.stats()
    return ins, (po, vo, st["max_speed"], orc.dt)


def _assert_same(got, want, nan=False):
    p, v, ms, dt = got
    po, vo, mso, dto = want
    assert np.array_equal(v, vo, equal_nan=nan), np.abs(v - vo).max()
    assert np.array_equal(p, po, equal_nan=nan), np.abs(p - po).max()
    assert ms == mso and dt == dto, (ms, mso, dt, dto)


def _restated(n, solid, ins, blend=1.0, **kw):
    U, UB, pos, pvel = ins
    return fr.flip_advect(n, solid, U, UB, pos, pvel, blend, **kw)


def _oracle(oracle, n, solid, pos, vel, blend=1.0, fields=None, pressure=True, **kw):
    orc = oracle.Oracle(n=n, **kw)
    orc.set_solid(solid)
    orc.set_particles(pos, vel)
    if blend < 1:
        orc.set_flip_blend(blend)
    orc.p2g(); orc.flags_index()
    if pressure:
        orc.pressure_pass()
    if fields is not None:
        orc.set_field(2, fields[0]); orc.set_field(3, fields[1])
    return orc


@pytest.mark.parametrize("blend", [1.0, 0.95, 0.0])
def test_matches_oracle_after_pressure_pass(fs, oracle, blend):
    n = 24
    pos = fs.water_cube_drop(n, 4, seed=0)
    vel = np.random.default_rng(1).standard_normal(pos.shape)
    solid = fr.default_solid(n)
    orc = _oracle(oracle, n, solid, pos, vel, blend)
    ins, want = _run_oracle(orc)
    assert np.abs(ins[0] - ins[1]).max() > 0            # a pass ran: the delta is not zero
    _assert_same(_restated(n, solid, ins, blend), want)


@pytest.mark.parametrize("blend", [1.0, 0.95, 0.0])
def test_obstacle_edges_and_aimed_particles(fs, oracle, blend):
    n = 32
    rng = np.random.default_rng(7)
    solid = fr.obstacle_solid(n)
    cube = fs.water_cube_drop(n, 4, seed=2)
    cube[:, 1] -= 4.0
    ep, ev = fr.edge_particles(n, rng)
    ap, av = fr.aimed(n, solid, rng)
    pos = np.concatenate([cube, ep, ap])
    vel = np.concatenate([rng.standard_normal(cube.shape) * 0.3, ev, av])
    orc = _oracle(oracle, n, solid, pos, vel, blend)
    ins, want = _run_oracle(orc)
    got = _restated(n, solid, ins, blend)
    _assert_same(got, want)
    # the scene takes the stuck branch and there truncation differs from floor, at negative coordinates
    k = len(cube) + len(ep)
    assert (got[1][k:] == 0).sum() > 50
    assert not np.array_equal(_restated(n, solid, ins, blend, trunc=np.floor)[1], want[1])


def test_adversarial_fields(fs, oracle):
    n = 32
    rng = np.random.default_rng(11)
    solid = fr.obstacle_solid(n)
    cube = fs.water_cube_drop(n, 2, seed=4)
    ep, ev = fr.edge_particles(n, rng)
    ap, av = fr.aimed(n, solid, rng, speed=600.0, spread=100.0)   # fast enough against the 1e3 fields to reach the faces
    pos = np.concatenate([cube, ep, ap, rng.uniform(-(n // 2) - 1, n // 2 + 1, size=(3000, 3))])
    vel = rng.standard_normal(pos.shape)
    vel[len(cube) + len(ep):len(cube) + len(ep) + len(ap)] = av
    fields = fr.adversarial_fields(n, rng)
    for blend in (1.0, 0.95, 0.0):
        orc = _oracle(oracle, n, solid, pos, vel, blend, fields=fields, pressure=False)
        ins, want = _run_oracle(orc)
        assert np.array_equal(ins[0], fields[0]) and np.array_equal(ins[1], fields[1])
        got = _restated(n, solid, ins, blend)
        _assert_same(got, want)
        # W moved by one on either side reads the 1e3 faces: no longer the oracle's result
        for wb in ((1, n - 3), (3, n - 3), (2, n - 2), (2, n - 4)):
            assert not np.array_equal(_restated(n, solid, ins, blend, wbound=wb)[1], want[1]), wb


def test_dx_and_max_dt(fs, oracle):
    """dt on both branches with dx != 1, and a state at rest: maxSpeed 0, dt = max_dt."""
    n = 24
    solid = fr.default_solid(n)
    pos = fs.water_cube_drop(n, 2, seed=5)
    for dx, max_dt, vscale, by_max_dt in ((0.5, 0.1, 0.1, True), (0.5, 0.1, 30.0, False), (2.0, 0.05, 5.0, True),
                                          (2.0, 0.05, 100.0, False), (1.0, 0.1, 0.0, True)):
        vel = np.random.default_rng(2).standard_normal(pos.shape) * vscale
        orc = _oracle(oracle, n, solid, pos, vel, pressure=False, dx=dx, max_dt=max_dt)
        z = np.zeros((3, n, n, n))
        f = fr.adversarial_fields(n, np.random.default_rng(3), outside=1.0) if vscale else (z, z)
        orc.set_field(2, f[0]); orc.set_field(3, f[1])
        ins, want = _run_oracle(orc)
        got = _restated(n, solid, ins, max_dt=max_dt, dx=dx)
        _assert_same(got, want)
        if vscale == 0:
            assert got[2] == 0 and got[3] == max_dt
        else:
            assert (got[3] == max_dt) == by_max_dt and got[3] == min(max_dt, dx / got[2]), (dx, max_dt, vscale, got[3])


def test_nan_velocity_does_not_set_dt(fs, oracle):
    n = 24
    solid = fr.default_solid(n)
    solid[12, 12, 12] = 1                              # world (0, 0, 0): where a device's NaN-to-int conversion would land
    pos = np.concatenate([fs.water_cube_drop(n, 2, seed=6), [[0.2, 0.9, -0.3]]])
    vel = np.random.default_rng(4).standard_normal(pos.shape)
    vel[-1] = np.nan
    orc = _oracle(oracle, n, solid, pos, vel, pressure=False)
    f = fr.adversarial_fields(n, np.random.default_rng(5))
    orc.set_field(2, f[0]); orc.set_field(3, f[1])
    ins, want = _run_oracle(orc)
    got = _restated(n, solid, ins)
    _assert_same(got, want, nan=True)
    assert np.isnan(got[0][-1]).all() and np.isnan(got[1][-1]).all()
    assert np.isfinite(got[0][:-1]).all() and got[2] == fr.max_speed(got[1][:-1]) > 0


def test_half_integer_ties_on_the_moved_axis(fs, oracle):
    """Moved coordinates exactly on x.5 between a fluid cell and a wall or obstacle cell, on both sides of zero: C round
    (half away from zero) decides stuck or free, and restatements with rint or floor(x + 0.5) no longer match."""
    n = 32
    rng = np.random.default_rng(12)
    solid = fr.tie_solid(n)
    pos, vel, ax = fr.tie_particles(n, solid, rng)
    U = fr.adversarial_fields(n, rng)[0]
    assert np.array_equal(fr.gather(n, U, U, pos, vel), vel)      # vel == velBefore: the gather leaves them exact
    orc = _oracle(oracle, n, solid, pos, vel, fields=(U, U), pressure=False, max_dt=fr.TIE_DT)
    ins, want = _run_oracle(orc)
    assert want[3] == fr.TIE_DT
    t = (pos + fr.TIE_DT * vel)[np.arange(len(pos)), ax]
    assert (t - np.floor(t) == 0.5).all() and (t < 0).sum() > 100 and (t > 0).sum() > 100
    got = _restated(n, solid, ins, max_dt=fr.TIE_DT)
    _assert_same(got, want)
    stuck = got[1][np.arange(len(pos)), ax] == 0
    assert stuck.any() and not stuck.all()
    neg, posi = fr.tie_changes(n, solid, U, pos, vel, ax, got, np.rint)
    assert neg > 0 and posi > 0, (neg, posi)
    neg, _ = fr.tie_changes(n, solid, U, pos, vel, ax, got, fr.floor_half_up)
    assert neg > 0


def test_one_face_inside_w_changes_exactly_its_readers(fs):
    n = 24
    rng = np.random.default_rng(8)
    solid = fr.default_solid(n)
    glo = -(n // 2)
    pos = rng.uniform(glo - 1, glo + n, size=(60000, 3))
    vel = rng.standard_normal(pos.shape)
    U, UB = fr.adversarial_fields(n, rng)
    base = fr.gather(n, U, UB, pos, vel)
    for a, face in ((0, (7, 9, 11)), (1, (2, 5, 21)), (2, (13, 3, 21)), (0, (22, 4, 4))):   # (22 = n - 2: read by cell n - 3 only)
        U2 = U.copy()
        U2[(a,) + face] += 1e12                     # large enough to show through the smallest nonzero weight
        got = fr.gather(n, U2, UB, pos, vel)
        # the cells whose getVelocity reads this face: c and c - e_a, those within W
        cells = [np.array(face), np.array(face) - np.eye(3, dtype=np.int64)[a]]
        cells = [c for c in cells if ((c >= 2) & (c <= n - 3)).all()]
        f = sr.c_round(pos).astype(np.int64) - glo
        reads = np.zeros(len(pos), dtype=bool)
        for c in cells:
            near = np.all(np.abs(f - c) <= 1, axis=1)
            w = np.ones(len(pos))
            for b in range(3):
                w *= sr.spline(pos[:, b] - (c[b] + glo))
            reads |= near & (w != 0)
        changed = np.any(got != base, axis=1)
        assert reads.sum() > 10
        assert np.array_equal(changed, reads), (a, face, (changed & ~reads).sum(), (reads & ~changed).sum())
        assert np.array_equal(got[:, [b for b in range(3) if b != a]], base[:, [b for b in range(3) if b != a]])


def test_one_face_outside_w_changes_nothing(fs):
    n = 24
    rng = np.random.default_rng(9)
    solid = fr.default_solid(n)
    glo = -(n // 2)
    pos = rng.uniform(glo - 1, glo + n, size=(20000, 3))
    vel = rng.standard_normal(pos.shape)
    U, UB = fr.adversarial_fields(n, rng)
    for blend in (1.0, 0.5):
        base = fr.flip_advect(n, solid, U, UB, pos, vel, blend)
        for a, face in ((0, (1, 9, 11)), (0, (n - 1, 5, 5)), (1, (5, 1, 7)), (1, (6, n - 1, 7)), (2, (8, 8, 1)),
                        (2, (4, 4, n - 1)), (0, (9, 1, 9)), (1, (9, 9, n - 2)), (2, (0, 0, 0))):
            for which in (0, 1):
                F = [U.copy(), UB.copy()]
                F[which][(a,) + face] += 1e6
                got = fr.flip_advect(n, solid, F[0], F[1], pos, vel, blend)
                for g, b in zip(got, base):
                    assert np.array_equal(g, b), (a, face, which)


def test_g2p_path_bit_in_the_header():
    """FLUID_PATH_G2P_TILES (flip_ref.PATH_G2P_TILES, the bit tests/test_gpu_g2p.py reads) is 1024 and shares no bit with the other path bits."""
    import os
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fluid_hip.h")
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FLUID_PATH_(\w+)\s+(\d+)", open(hdr).read())}
    assert bits["G2P_TILES"] == fr.PATH_G2P_TILES == 1024
    vals = list(bits.values())
    assert all(v & (v - 1) == 0 for v in vals) and len(set(vals)) == len(vals), bits
