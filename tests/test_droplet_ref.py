"""tests/droplet_ref.py checked on the CPU: the labelling against a second, independent one; claim_rule on every hand pocket
with the verdict written out in the builder; and the condition on the scenes themselves — the reference CG, uncapped, reaches
half of both backward-error bars on every pocket of every scene the GPU module uses (if a shape could not, the shape would have
to change, never the bar).  The iteration counts of the sealed pockets are printed: k_drop_solve's cap is sized from them."""
import numpy as np
import pytest

import droplet_ref as dr
import pressure_system as ps

GPU_SCENES = [k for k in dr.SCENES]


def _second_labelling(mask):
    try:
        from scipy import ndimage
        lab, k = ndimage.label(mask)          # default structure: 6-connectivity
        return lab.reshape(-1) - 1, k
    except ImportError:
        n = mask.shape[0]
        parent = np.arange(n ** 3)

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        flat = mask.reshape(-1)
        for a in np.flatnonzero(flat):
            for s in (n * n, n, 1):
                if flat[a + s]:
                    ra, rb = find(a), find(a + s)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
        out = np.full(n ** 3, -1)
        roots = {}
        for a in np.flatnonzero(flat):
            out[a] = roots.setdefault(find(a), len(roots))
        return out, len(roots)


@pytest.mark.parametrize("seed,fill", [(0, 0.15), (1, 0.3), (2, 0.5), (3, 0.7)])
def test_label_against_a_second_labelling(seed, fill):
    n = 12
    rng = np.random.default_rng(seed)
    mask = np.zeros((n, n, n), dtype=bool)
    mask[1:-1, 1:-1, 1:-1] = rng.random((n - 2,) * 3) < fill
    comps = dr.label(mask)
    other, k = _second_labelling(mask)
    assert len(comps) == k
    assert np.array_equal(comps.ids >= 0, mask.reshape(-1))
    # the same partition: a one-to-one map between the two numberings
    pairs = set(zip(comps.ids[comps.ids >= 0].tolist(), other[comps.ids >= 0].tolist()))
    assert len(pairs) == k and len({a for a, _ in pairs}) == k and len({b for _, b in pairs}) == k
    for c in range(k):
        cells = np.flatnonzero(comps.ids == c)
        assert np.array_equal(comps.cells[c], cells) and comps.sizes[c] == len(cells) and comps.first[c] == cells[0]
    assert np.all(np.diff(comps.first) > 0)           # numbered by first cell


built = dr.built


@pytest.mark.parametrize("name", [k for k in dr.SCENES if k != "overflow"])
def test_claim_rule_on_the_hand_cases(name):
    c, s, notes, comps, sys_ = built(name)
    n = notes["n"]
    assert np.array_equal(s == 1, (dr.shell_solid(n) == 1) | (s == 1)) and np.all(s[dr.shell_solid(n) == 1] == 1)
    assert np.array_equal(np.sort(sys_.cells[sys_.in_system]), np.flatnonzero(comps.ids >= 0))   # two statements of "unknown"
    want = dr.expected_claims(comps, notes)
    got = dr.claim_rule(comps, n)
    if "cuts" in notes:     # a decomposed run: claimed when some block owns every cell; on one GPU all these pockets are claimed
        assert got[list(want)].all()
        per_block = [dr.claim_rule(comps, n, own) for own in dr.block_masks(n, notes["cuts"])]
        got = np.any(per_block, axis=0)
        assert np.sum(per_block, axis=0).max() == 1
    for p in notes["pockets"]:
        comp = int(comps.ids[p["cells"][0]])
        assert bool(got[comp]) == p["claim"], f"{name} / {p['name']}: {p['why']}"
    # everything that is no hand pocket is the pool (if any) and is not claimed
    rest = [k for k in range(len(comps)) if k not in want]
    assert len(rest) == (0 if name == "all_pockets" else 1), rest
    assert not got[rest].any() and all(comps.sizes[k] >= 576 for k in rest)
    for cell in notes.get("walled", []):
        assert c.reshape(-1)[cell] > 0 and comps.ids[cell] < 0
    # own: a pocket with one cell outside the owned set must not be claimed
    claimed = np.flatnonzero(got)
    if len(claimed):
        own = np.ones(n ** 3, dtype=bool)
        own[comps.cells[claimed[0]][-1]] = False
        got2 = dr.claim_rule(comps, n, own)
        assert not got2[claimed[0]] and np.array_equal(got2[claimed[1:]], got[claimed[1:]])


def test_overflow_scene_overflows():
    c, s, notes, comps, sys_ = built("overflow")
    n = notes["n"]
    assert notes["overflow"] and (comps.sizes == 1).all() and len(comps) > dr.DROP_CAP
    assert dr.claim_rule(comps, n).all()
    x, r = np.divmod(comps.first, n * n)
    y, z = np.divmod(r, n)
    nc = n // dr.CORE
    block = ((x // 8) * nc + y // 8) * nc + z // 8
    per_range = np.bincount(block % dr.DROP_NCTR, minlength=dr.DROP_NCTR)
    assert per_range.max() > dr.DROP_CAP // dr.DROP_NCTR
    assert np.bincount(block).max() == 256


def test_crowd_scene_is_one_block():
    c, s, notes, comps, sys_ = built("crowd")
    firsts = np.array([p["cells"][0] for p in notes["pockets"]])
    n = notes["n"]
    cores = {(f // (n * n) // 8, (f // n) % n // 8, f % n // 8) for f in firsts.tolist()}
    assert len(firsts) == 256 and len(cores) == 1


@pytest.mark.parametrize("name", GPU_SCENES)
def test_reference_cg_reaches_half_the_bars_on_every_pocket(name):
    """b: a seeded float32 vector over the unknowns.  Every component of at most 64 cells, solved alone by the uncapped
    reference CG at the product's tolerance, must reach eta <= ETA_BAR / 2 and omega <= OMEGA_BAR / 2."""
    c, s, notes, comps, sys_ = built(name)
    rng = np.random.default_rng(7)
    b = rng.standard_normal(sys_.size).astype(np.float32).astype(np.float64)
    row_of = np.full(notes["n"] ** 3, -1, dtype=np.int64)
    row_of[sys_.cells] = np.arange(sys_.size)
    sealed = {int(comps.ids[p["cells"][0]]): p["name"] for p in notes["pockets"] if p["sealed"]}
    small = np.flatnonzero(comps.sizes <= dr.POCKET_MAX)
    if notes["overflow"]:
        small = small[:: 97]                          # single cells, all alike: every 97th
    p = np.zeros(sys_.size)
    worst = (0.0, 0.0, 0)
    for k in small:
        rows = row_of[comps.cells[k]]
        A = dr.pocket_matrix(sys_, rows)
        x, it, rel = dr.pocket_cg(A, b[rows])
        p[rows] = x
        res = ps.residual(sys_, b, p, rows)
        worst = (max(worst[0], res["eta"]), max(worst[1], res["omega"]), max(worst[2], it))
        if k in sealed:
            _, it_cap, rel_cap = dr.pocket_cg(A, b[rows], cap=len(rows) + 8)
            print(f"{name} / {sealed[k]}: n {len(rows)} iterations {it} (old cap n + 8 = {len(rows) + 8}: stopped after {it_cap}"
                  f" at {rel_cap:.1e}) eta {res['eta']:.1e} omega {res['omega']:.1e} cond {np.linalg.cond(A / np.sqrt(np.outer(np.diag(A), np.diag(A)))):.0f}")
        assert res["eta"] <= ps.ETA_BAR / 2 and res["omega"] <= ps.OMEGA_BAR / 2, (name, k, len(rows), it, res["eta"], res["omega"])
    print(f"{name}: {len(small)} pockets, worst eta {worst[0]:.1e} omega {worst[1]:.1e}, most iterations {worst[2]}")


def test_sealed_pockets_stay_under_the_solve_cap():
    """The sealed pockets over 60 right-hand sides of three kinds (white noise; noise over four decades; one loaded cell):
    the uncapped reference CG's largest iteration count per shape — what k_drop_solve's cap is sized from.  In float64 the
    sealed paths need up to 2 n iterations (exact arithmetic: n), the branched ones about 60 whatever their size; the old cap
    n + 8 was short for four of the five shapes.  The cap leaves at least 8 iterations over the largest count: the device sums
    in another order."""
    c, s, notes, comps, sys_ = built("sealed")
    row_of = np.full(notes["n"] ** 3, -1, dtype=np.int64)
    row_of[sys_.cells] = np.arange(sys_.size)
    over_old = 0
    for p in notes["pockets"]:
        rows = row_of[p["cells"]]
        A, n = dr.pocket_matrix(sys_, rows), len(rows)
        its = []
        for seed in range(60):
            rng = np.random.default_rng(seed)
            if seed % 3 == 0:
                b = rng.standard_normal(n)
            elif seed % 3 == 1:
                b = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)
            else:
                b = 1e-6 * rng.standard_normal(n)
                b[rng.integers(n)] = 1.0
            its.append(dr.pocket_cg(A, b.astype(np.float32).astype(np.float64))[1])
        print(f"{p['name']}: n {n} most iterations {max(its)} (old cap {n + 8}, cap {dr.drop_solve_cap(n)})")
        over_old += max(its) > n + 8
        assert max(its) + 8 <= dr.drop_solve_cap(n), p["name"]
    assert over_old >= 2       # the scenes do exercise the cap
