// fluid_sdf_grids_merge under AddressSanitizer + UBSan (tests/test_sdf_merge.py builds and runs this with g++ together with
// vdb_sdf_writer.cpp): hand-made parts that overlap in some leaves and not in others, partial edge leaves, empty parts; the merge
// against the per-voxel rule restated here on dense arrays; the count-only call; every refused kind of input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fluid_hip.h"

static int fail(const char* what)
{
    std::fprintf(stderr, "FAILED: %s\n", what);
    return 1;
}

struct List {
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
    fluid_sdf_grid_t g;
    void bind(int n, float bg)
    {
        g.n = n;
        g.n_leaves = (int32_t)(origin.size() / 3);
        g.background = bg, g.radius = 1.5f, g.half_width = 2.5f;
        g.origin = origin.data(), g.values = values.data(), g.active = active.data();
    }
};

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the leaves whose running number is congruent to `phase` modulo `every` (and the corner leaves), in-grid voxels at random:
// active with one of a few values (so that ties occur), inactive -bg or inactive +bg
static void make(int n, int every, int phase, uint32_t seed, float bg, List& L)
{
    const int lo = -(n / 2), hi = lo + n - 1, l0 = lo & ~7, l1 = hi & ~7;
    uint32_t s = seed;
    int count = 0;
    for (int ox = l0; ox <= l1; ox += 8)
        for (int oy = l0; oy <= l1; oy += 8)
            for (int oz = l0; oz <= l1; oz += 8) {
                const bool corner = (ox == l0 || ox == l1) && (oy == l0 || oy == l1) && (oz == l0 || oz == l1);
                if (count++ % every != phase && !corner) continue;
                float v[512];
                uint64_t m[8] = {};
                for (int off = 0; off < 512; ++off) {
                    const int x = ox + (off >> 6), y = oy + ((off >> 3) & 7), z = oz + (off & 7);
                    const bool in = x >= lo && x <= hi && y >= lo && y <= hi && z >= lo && z <= hi;
                    const uint32_t r = rnd(s) >> 8;
                    v[off] = bg;
                    if (!in) continue;
                    const int kind = (int)(r % 7);
                    if (kind == 0) v[off] = -bg;
                    else if (kind < 4) {
                        v[off] = bg * ((float)((r >> 3) % 5) / 4.f - 0.75f);   // -0.75 bg .. +0.25 bg in five steps
                        m[off >> 6] |= 1ull << (off & 63);
                    }
                }
                L.origin.insert(L.origin.end(), {ox, oy, oz});
                L.values.insert(L.values.end(), v, v + 512);
                L.active.insert(L.active.end(), m, m + 8);
            }
    L.bind(n, bg);
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main()
{
    const float bg = 2.5f;
    for (int n : {8, 25, 40}) {
        List P[4];
        make(n, 2, 0, 11u + (uint32_t)n, bg, P[0]);
        make(n, 3, 1, 22u + (uint32_t)n, bg, P[1]);
        make(n, 1, 0, 33u + (uint32_t)n, bg, P[2]);
        P[3].bind(n, bg);   // an empty part: n_leaves == 0 behind NULL pointers
        P[3].g.origin = nullptr, P[3].g.values = nullptr, P[3].g.active = nullptr;
        const fluid_sdf_grid_t parts[4] = {P[0].g, P[1].g, P[3].g, P[2].g};
        const int64_t k = fluid_sdf_grids_merge(parts, 4, 0, nullptr, nullptr, nullptr);
        if (k != P[2].g.n_leaves) return fail("count");   // P[2] lists every leaf of the grid
        std::vector<int32_t> org(3 * (size_t)k);
        std::vector<float> val(512 * (size_t)k);
        std::vector<uint64_t> act(8 * (size_t)k);
        if (fluid_sdf_grids_merge(parts, 4, k, org.data(), val.data(), act.data()) != k) return fail("merge");
        if (std::memcmp(org.data(), P[2].origin.data(), org.size() * 4) != 0) return fail("origins");
        // the rule, voxel by voxel on dense arrays
        const size_t nc = (size_t)n * n * n;
        std::vector<float> ev(nc, bg), dv(nc), pv(nc);
        std::vector<uint8_t> ea(nc, 0), da(nc), pa(nc);
        for (const fluid_sdf_grid_t& g : parts) {
            if (fluid_sdf_to_dense(&g, pv.data(), pa.data()) != FLUID_OK) return fail("to_dense of a part");
            for (size_t c = 0; c < nc; ++c) {
                if (!ea[c] && same_bits(ev[c], -bg)) continue;
                if (!pa[c]) {
                    if (same_bits(pv[c], -bg)) ev[c] = -bg, ea[c] = 0;
                } else if (!ea[c] || pv[c] < ev[c]) ev[c] = pv[c], ea[c] = 1;
            }
        }
        const fluid_sdf_grid_t merged = {n, (int32_t)k, bg, 1.5f, 2.5f, org.data(), val.data(), act.data()};
        if (fluid_sdf_to_dense(&merged, dv.data(), da.data()) != FLUID_OK) return fail("to_dense of the merge");
        if (std::memcmp(dv.data(), ev.data(), nc * 4) != 0 || std::memcmp(da.data(), ea.data(), nc) != 0) return fail("the merged voxels");
        // one part alone, and empty parts only
        std::vector<float> v1(P[0].values.size());
        std::vector<int32_t> o1(P[0].origin.size());
        std::vector<uint64_t> a1(P[0].active.size());
        if (fluid_sdf_grids_merge(&P[0].g, 1, P[0].g.n_leaves, o1.data(), v1.data(), a1.data()) != P[0].g.n_leaves) return fail("one part");
        if (o1 != P[0].origin || std::memcmp(v1.data(), P[0].values.data(), v1.size() * 4) != 0 || a1 != P[0].active) return fail("one part: the records");
        const fluid_sdf_grid_t none[2] = {P[3].g, P[3].g};
        if (fluid_sdf_grids_merge(none, 2, 0, o1.data(), v1.data(), a1.data()) != 0) return fail("empty parts");
        // refusals: nothing is written (the arrays are exactly as large as the merge needs: a write past them is the sanitizer's)
        const std::vector<int32_t> org0 = org;
        const std::vector<float> val0 = val;
        const std::vector<uint64_t> act0 = act;
        auto refused = [&](const fluid_sdf_grid_t* ps, int np, int64_t cap) {
            return fluid_sdf_grids_merge(ps, np, cap, org.data(), val.data(), act.data()) == -FLUID_ERR_ARG && org == org0 &&
                   std::memcmp(val.data(), val0.data(), val.size() * 4) == 0 && act == act0;
        };
        auto bad_list = [&](const fluid_sdf_grid_t* ps, int np) {   // refused whatever the capacity, and by the count-only call too
            return refused(ps, np, k) && fluid_sdf_grids_merge(ps, np, 0, nullptr, nullptr, nullptr) == -FLUID_ERR_ARG;
        };
        if (!refused(parts, 4, k - 1)) return fail("a capacity one too small accepted");
        if (!bad_list(parts, 0) || !bad_list(nullptr, 4)) return fail("no parts accepted");
        if (fluid_sdf_grids_merge(parts, 4, k, org.data(), nullptr, act.data()) != -FLUID_ERR_ARG) return fail("some output arrays only accepted");
        fluid_sdf_grid_t bad[4] = {parts[0], parts[1], parts[2], parts[3]};
        bad[1].n = n + 1;
        if (!bad_list(bad, 4)) return fail("different n accepted");
        bad[1] = parts[1], bad[1].background = 2.75f;
        if (!bad_list(bad, 4)) return fail("different background accepted");
        bad[1] = parts[1], bad[2].radius = 1.25f;
        if (!bad_list(bad, 4)) return fail("different radius accepted (on an empty part)");
        bad[2] = parts[2], bad[3].half_width = 2.0f;
        if (!bad_list(bad, 4)) return fail("different half width accepted");
        bad[3] = parts[3];
        List B = P[1];
        B.bind(n, bg);
        bad[1] = B.g;
        B.origin[2] += 4;
        if (!bad_list(bad, 4)) return fail("unaligned origin accepted");
        B.origin = P[1].origin;
        B.origin[0] = (-(n / 2) & ~7) - 8;
        if (!bad_list(bad, 4)) return fail("outside origin accepted");
        if (B.g.n_leaves > 1) {
            B.origin = P[1].origin;
            for (int a = 0; a < 3; ++a) B.origin[3 + a] = B.origin[a];
            if (!bad_list(bad, 4)) return fail("duplicate origin accepted");
        }
        B.origin = P[1].origin;
        int off = 0;
        const size_t last = (size_t)B.g.n_leaves - 1;
        while (off < 512 && ((B.active[8 * last + (off >> 6)] >> (off & 63)) & 1)) ++off;
        if (off == 512) return fail("no inactive voxel to spoil");
        B.values[512 * last + off] = 0.75f;
        if (!bad_list(bad, 4)) return fail("an inactive value that is neither +bg nor -bg accepted");
        B.values = P[1].values;
        bad[1].active = nullptr;
        if (!bad_list(bad, 4)) return fail("null mask array accepted");
        bad[1] = B.g;
        if (fluid_sdf_grids_merge(bad, 4, k, org.data(), val.data(), act.data()) != k) return fail("the restored parts do not merge");
    }
    std::puts("host sanitizer run (sdf merge): ok");
    return 0;
}
