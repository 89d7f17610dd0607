// fluid_sdf_attr_grids_merge under AddressSanitizer + UBSan (tests/test_sdf_attr_merge.py builds and runs this with g++ together
// with vdb_sdf_writer.cpp): hand-made rank records that overlap in some leaves and not in others, partial edge leaves, an empty
// part; the merge against the per-voxel rule restated here on dense arrays, its geometry against fluid_sdf_grids_merge; the
// count-only call; every refused kind of input.  The records are made so that dist2 orders the parts as the values do (the value
// is a monotone function of dist2), with ties on dist2 and on (dist2, id).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
    std::vector<uint32_t> id;
    std::vector<float> velocity, dist2;
    fluid_sdf_grid_t g;
    fluid_sdf_attr_part_t a;
    void bind(int n, float bg)
    {
        g.n = n;
        g.n_leaves = (int32_t)(origin.size() / 3);
        g.background = bg, g.radius = 1.5f, g.half_width = 2.5f;
        g.origin = origin.data(), g.values = values.data(), g.active = active.data();
        a.n_leaves = g.n_leaves;
        a.id = id.data(), a.velocity = velocity.data(), a.dist2 = dist2.data();
    }
};

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the leaves whose running number is congruent to `phase` modulo `every` (and the corner leaves), in-grid voxels at random: active
// with one of five squared distances (so that ties occur) and one of three ids from id0 on, inactive -bg or inactive +bg
static void make(int n, int every, int phase, uint32_t seed, float bg, uint32_t id0, List& L)
{
    const int lo = -(n / 2), hi = lo + n - 1, l0 = lo & ~7, l1 = hi & ~7;
    const float inf = std::numeric_limits<float>::infinity();
    uint32_t s = seed;
    int count = 0;
    for (int ox = l0; ox <= l1; ox += 8)
        for (int oy = l0; oy <= l1; oy += 8)
            for (int oz = l0; oz <= l1; oz += 8) {
                const bool corner = (ox == l0 || ox == l1) && (oy == l0 || oy == l1) && (oz == l0 || oz == l1);
                if (count++ % every != phase && !corner) continue;
                float v[512], d[512], w[1536];
                uint32_t ids[512];
                uint64_t m[8] = {};
                for (int off = 0; off < 512; ++off) {
                    const int x = ox + (off >> 6), y = oy + ((off >> 3) & 7), z = oz + (off & 7);
                    const bool in = x >= lo && x <= hi && y >= lo && y <= hi && z >= lo && z <= hi;
                    const uint32_t r = rnd(s) >> 8;
                    v[off] = bg, d[off] = inf, ids[off] = FLUID_SDF_NO_ID;
                    w[off] = w[512 + off] = w[1024 + off] = 0.0f;
                    if (!in) continue;
                    const int kind = (int)(r % 7);
                    if (kind == 0) v[off] = -bg;
                    else if (kind < 4) {
                        const int step = (int)((r >> 3) % 5);
                        d[off] = 1.0f + 0.5f * (float)step;                  // the squared distance ...
                        v[off] = std::sqrt(d[off]) - 1.5f;                   // ... and the value it gives: monotone, well inside the band
                        ids[off] = id0 + (r >> 7) % 3;
                        w[off] = (float)ids[off] + 0.25f, w[512 + off] = -(float)step, w[1024 + off] = (float)(seed & 255u);
                        m[off >> 6] |= 1ull << (off & 63);
                    }
                }
                L.origin.insert(L.origin.end(), {ox, oy, oz});
                L.values.insert(L.values.end(), v, v + 512);
                L.active.insert(L.active.end(), m, m + 8);
                L.id.insert(L.id.end(), ids, ids + 512);
                L.velocity.insert(L.velocity.end(), w, w + 1536);
                L.dist2.insert(L.dist2.end(), d, d + 512);
            }
    L.bind(n, bg);
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main()
{
    const float bg = 2.5f;
    for (int n : {8, 25, 40}) {
        List P[4];
        make(n, 2, 0, 11u + (uint32_t)n, bg, 10u, P[0]);
        make(n, 3, 1, 22u + (uint32_t)n, bg, 11u, P[1]);   // ids overlap with the other parts': ties on (dist2, id) occur
        make(n, 1, 0, 33u + (uint32_t)n, bg, 9u, P[2]);
        P[3].bind(n, bg);   // an empty part: n_leaves == 0 behind NULL pointers
        P[3].g.origin = nullptr, P[3].g.values = nullptr, P[3].g.active = nullptr;
        P[3].a.id = nullptr, P[3].a.velocity = nullptr, P[3].a.dist2 = nullptr;
        const fluid_sdf_grid_t parts[4] = {P[0].g, P[1].g, P[3].g, P[2].g};
        const fluid_sdf_attr_part_t recs[4] = {P[0].a, P[1].a, P[3].a, P[2].a};
        const List* src[4] = {&P[0], &P[1], &P[3], &P[2]};
        const int64_t k = fluid_sdf_attr_grids_merge(parts, recs, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (k != P[2].g.n_leaves) return fail("count");   // P[2] lists every leaf of the grid
        std::vector<int32_t> org(3 * (size_t)k), org2(3 * (size_t)k);
        std::vector<float> val(512 * (size_t)k), val2(512 * (size_t)k), vel(1536 * (size_t)k);
        std::vector<uint64_t> act(8 * (size_t)k), act2(8 * (size_t)k);
        std::vector<uint32_t> id(512 * (size_t)k);
        if (fluid_sdf_attr_grids_merge(parts, recs, 4, k, org.data(), val.data(), act.data(), id.data(), vel.data()) != k) return fail("merge");
        if (fluid_sdf_grids_merge(parts, 4, k, org2.data(), val2.data(), act2.data()) != k) return fail("plain merge");
        if (org != org2 || act != act2 || std::memcmp(val.data(), val2.data(), val.size() * 4) != 0) return fail("the geometry is not the plain merge's");
        // the rule, voxel by voxel: every leaf of the grid is leaf l of P[2] and of the merge
        std::vector<size_t> cur(4, 0);
        int ties = 0, id_ties = 0;
        for (int64_t l = 0; l < k; ++l) {
            const int32_t* o = org.data() + 3 * l;
            for (int off = 0; off < 512; ++off) {
                int best = -1;
                size_t bl = 0;
                for (int p = 0; p < 4; ++p) {
                    const List& L = *src[p];
                    if (cur[p] >= (size_t)L.g.n_leaves || std::memcmp(L.origin.data() + 3 * cur[p], o, 12) != 0) continue;
                    const size_t i = 512 * cur[p] + off;
                    if (!((L.active[8 * cur[p] + (off >> 6)] >> (off & 63)) & 1)) continue;
                    if (best >= 0) {
                        const List& B = *src[best];
                        const size_t j = 512 * bl + off;
                        if (L.dist2[i] == B.dist2[j]) ++ties, id_ties += L.id[i] == B.id[j];
                        if (!(L.dist2[i] < B.dist2[j] || (L.dist2[i] == B.dist2[j] && L.id[i] < B.id[j]))) continue;
                    }
                    best = p, bl = cur[p];
                }
                const size_t m = 512 * (size_t)l + off;
                const bool on = (act[8 * (size_t)l + (off >> 6)] >> (off & 63)) & 1;
                uint32_t eid = FLUID_SDF_NO_ID;
                float ev[3] = {0.0f, 0.0f, 0.0f};
                if (on) {
                    if (best < 0) return fail("an active merged voxel no part holds active");
                    const List& B = *src[best];
                    eid = B.id[512 * bl + off];
                    for (int a = 0; a < 3; ++a) ev[a] = B.velocity[1536 * bl + 512 * a + off];
                    if (!same_bits(val[m], B.values[512 * bl + off])) return fail("the closest part's value");
                }
                if (id[m] != eid) return fail("a merged id");
                for (int a = 0; a < 3; ++a)
                    if (!same_bits(vel[1536 * (size_t)l + 512 * a + off], ev[a])) return fail("a merged velocity");
            }
            for (int p = 0; p < 4; ++p)
                if (cur[p] < (size_t)src[p]->g.n_leaves && std::memcmp(src[p]->origin.data() + 3 * cur[p], o, 12) == 0) cur[p]++;
        }
        if (ties == 0 || id_ties == 0) return fail("the input has no tie on dist2, or none on (dist2, id)");
        // one part alone, and empty parts only
        {
            const List& A = P[0];
            const size_t k1 = (size_t)A.g.n_leaves;
            std::vector<int32_t> o1(3 * k1);
            std::vector<float> v1(512 * k1), w1(1536 * k1);
            std::vector<uint64_t> a1(8 * k1);
            std::vector<uint32_t> i1(512 * k1);
            if (fluid_sdf_attr_grids_merge(&A.g, &A.a, 1, (int64_t)k1, o1.data(), v1.data(), a1.data(), i1.data(), w1.data()) != (int64_t)k1) return fail("one part");
            if (o1 != A.origin || a1 != A.active || i1 != A.id || std::memcmp(v1.data(), A.values.data(), v1.size() * 4) != 0 ||
                std::memcmp(w1.data(), A.velocity.data(), w1.size() * 4) != 0)
                return fail("one part: the records");
            const fluid_sdf_grid_t none[2] = {P[3].g, P[3].g};
            const fluid_sdf_attr_part_t nrec[2] = {P[3].a, P[3].a};
            if (fluid_sdf_attr_grids_merge(none, nrec, 2, 0, o1.data(), v1.data(), a1.data(), i1.data(), w1.data()) != 0) return fail("empty parts");
        }
        // refusals: nothing is written (the arrays are exactly as large as the merge needs: a write past them is the sanitizer's)
        const std::vector<int32_t> org0 = org;
        const std::vector<float> val0 = val, vel0 = vel;
        const std::vector<uint64_t> act0 = act;
        const std::vector<uint32_t> id0 = id;
        auto refused = [&](const fluid_sdf_grid_t* ps, const fluid_sdf_attr_part_t* as, int np, int64_t cap) {
            return fluid_sdf_attr_grids_merge(ps, as, np, cap, org.data(), val.data(), act.data(), id.data(), vel.data()) == -FLUID_ERR_ARG &&
                   org == org0 && act == act0 && id == id0 && std::memcmp(val.data(), val0.data(), val.size() * 4) == 0 &&
                   std::memcmp(vel.data(), vel0.data(), vel.size() * 4) == 0;
        };
        auto bad_list = [&](const fluid_sdf_grid_t* ps, const fluid_sdf_attr_part_t* as, int np) {   // whatever the capacity, and count-only too
            return refused(ps, as, np, k) &&
                   fluid_sdf_attr_grids_merge(ps, as, np, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == -FLUID_ERR_ARG;
        };
        if (!refused(parts, recs, 4, k - 1)) return fail("a capacity one too small accepted");
        if (!bad_list(parts, recs, 0) || !bad_list(nullptr, recs, 4) || !bad_list(parts, nullptr, 4)) return fail("no parts accepted");
        if (fluid_sdf_attr_grids_merge(parts, recs, 4, k, org.data(), val.data(), act.data(), nullptr, vel.data()) != -FLUID_ERR_ARG)
            return fail("some output arrays only accepted");
        fluid_sdf_grid_t bad[4] = {parts[0], parts[1], parts[2], parts[3]};
        fluid_sdf_attr_part_t brec[4] = {recs[0], recs[1], recs[2], recs[3]};
        bad[1].n = n + 1;
        if (!bad_list(bad, recs, 4)) return fail("different n accepted");
        bad[1] = parts[1], bad[2].radius = 1.25f;
        if (!bad_list(bad, recs, 4)) return fail("different radius accepted (on an empty part)");
        bad[2] = parts[2];
        List B = P[1];
        B.bind(n, bg);
        bad[1] = B.g, brec[1] = B.a;
        B.origin[2] += 4;
        if (!bad_list(bad, brec, 4)) return fail("unaligned origin accepted");
        B.origin = P[1].origin;
        int off = 0;
        const size_t last = (size_t)B.g.n_leaves - 1;
        while (off < 512 && ((B.active[8 * last + (off >> 6)] >> (off & 63)) & 1)) ++off;
        if (off == 512) return fail("no inactive voxel to spoil");
        B.values[512 * last + off] = 0.75f;
        if (!bad_list(bad, brec, 4)) return fail("an inactive value that is neither +bg nor -bg accepted");
        B.values = P[1].values;
        brec[1].n_leaves -= 1;
        if (!bad_list(bad, brec, 4)) return fail("a record of another leaf count accepted");
        brec[1] = B.a, brec[1].dist2 = nullptr;
        if (!bad_list(bad, brec, 4)) return fail("leaves without dist2 accepted");
        brec[1] = B.a, brec[1].id = nullptr;
        if (!bad_list(bad, brec, 4)) return fail("leaves without ids accepted");
        brec[1] = B.a, brec[1].velocity = nullptr;
        if (!bad_list(bad, brec, 4)) return fail("leaves without velocities accepted");
        brec[1] = B.a;
        int on = 0;
        while (on < 512 && !((B.active[8 * last + (on >> 6)] >> (on & 63)) & 1)) ++on;
        if (on == 512) return fail("no active voxel to spoil");
        const float d_keep = B.dist2[512 * last + on];
        B.dist2[512 * last + on] = std::numeric_limits<float>::infinity();
        if (!bad_list(bad, brec, 4)) return fail("an active voxel with an infinite dist2 accepted");
        B.dist2[512 * last + on] = std::numeric_limits<float>::quiet_NaN();
        if (!bad_list(bad, brec, 4)) return fail("an active voxel with a NaN dist2 accepted");
        B.dist2[512 * last + on] = d_keep;
        const uint32_t i_keep = B.id[512 * last + on];
        B.id[512 * last + on] = FLUID_SDF_NO_ID;
        if (!bad_list(bad, brec, 4)) return fail("an active voxel without an id accepted");
        B.id[512 * last + on] = i_keep;
        // the closest part does not hold the smallest value: find a voxel two parts hold active with different dist2, swap the claim
        bool spoiled = false;
        for (size_t lb = 0; lb < (size_t)B.g.n_leaves && !spoiled; ++lb)
            for (size_t l2 = 0; l2 < (size_t)P[2].g.n_leaves && !spoiled; ++l2) {
                if (std::memcmp(B.origin.data() + 3 * lb, P[2].origin.data() + 3 * l2, 12) != 0) continue;
                for (int v = 0; v < 512 && !spoiled; ++v) {
                    const bool a1 = (B.active[8 * lb + (v >> 6)] >> (v & 63)) & 1, a2 = (P[2].active[8 * l2 + (v >> 6)] >> (v & 63)) & 1;
                    if (!a1 || !a2 || !(B.dist2[512 * lb + v] > P[2].dist2[512 * l2 + v])) continue;
                    const float keep = B.dist2[512 * lb + v];
                    B.dist2[512 * lb + v] = 0.25f;   // closer than anything, with the larger value
                    if (!bad_list(bad, brec, 4)) return fail("a dist2 that contradicts the values accepted");
                    B.dist2[512 * lb + v] = keep;
                    spoiled = true;
                }
            }
        if (!spoiled) return fail("no voxel to contradict");
        if (fluid_sdf_attr_grids_merge(bad, brec, 4, k, org.data(), val.data(), act.data(), id.data(), vel.data()) != k) return fail("the restored parts do not merge");
        if (org != org0 || id != id0) return fail("the restored parts merge differently");
    }
    std::puts("host sanitizer run (sdf attribute merge): ok");
    return 0;
}
