// Stand-alone driver of the host grown level-set filter for the sanitizer build (tests/test_sdf_grow_host.py): two balls at n = 20,
// where the grid [-10, 9] ends inside a leaf on both sides — one in the middle of leaf (0, 0, 0), which lists one leaf and grows
// through all six faces, one cut by the grid's lo face — with an id and a velocity per active voxel go through
// fluid_sdf_filter_grown, with and without attributes, for offsets in both directions up to the limit of 4 dx.  What the
// definition promises is checked on every result (the bytes themselves are pinned by the Python tests): ascending origins on the
// 8-grid, inactive voxels at +-bg, nothing active outside the grid, active <=> has an id, an inherited id is one of the input's;
// then the count-only form, exact capacities, and the refusals, none of which may write.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "fluid_hip.h"

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);  \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main()
{
    const int n = 20, lo = -(n / 2), hi = lo + n - 1, L0 = lo & ~7;
    const float bg = 2.0f, R = 2.0f, w = 2.0f;
    const float centre[2][3] = {{3.5f, 3.5f, 3.5f}, {(float)lo + 0.4f, -3.2f, 2.1f}};
    std::vector<int32_t> origin;
    std::vector<float> values, velocity;
    std::vector<uint64_t> active;
    std::vector<uint32_t> ids;
    std::set<uint32_t> given;
    for (int ox = L0; ox <= hi; ox += 8)
        for (int oy = L0; oy <= hi; oy += 8)
            for (int oz = L0; oz <= hi; oz += 8) {
                float v[512], vel[1536] = {};
                uint32_t id[512];
                uint64_t m[8] = {};
                bool listed = false;
                for (int off = 0; off < 512; ++off) {
                    const int c[3] = {ox + (off >> 6), oy + ((off >> 3) & 7), oz + (off & 7)};
                    float d = bg;
                    int who = -1;
                    bool in = true;
                    for (int a = 0; a < 3; ++a) in = in && c[a] >= lo && c[a] <= hi;
                    if (in)
                        for (int p = 0; p < 2; ++p) {
                            const float* q = centre[p];
                            const float e = std::sqrt((c[0] - q[0]) * (c[0] - q[0]) + (c[1] - q[1]) * (c[1] - q[1]) + (c[2] - q[2]) * (c[2] - q[2])) - R;
                            if (e < d) d = e, who = p;
                        }
                    id[off] = FLUID_SDF_NO_ID;
                    if (d <= -bg) d = -bg;
                    else if (d < bg) {
                        m[off >> 6] |= 1ull << (off & 63);
                        id[off] = 1000u * (uint32_t)(who + 1) + (uint32_t)off;
                        given.insert(id[off]);
                        for (int a = 0; a < 3; ++a) vel[512 * a + off] = (float)(who + 1) + 0.25f * (float)a;
                    }
                    v[off] = d;
                    listed = listed || d != bg;
                }
                if (!listed) continue;
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
                ids.insert(ids.end(), id, id + 512);
                velocity.insert(velocity.end(), vel, vel + 1536);
            }
    fluid_sdf_grid_t g{n, (int32_t)(origin.size() / 3), bg, R, w, origin.data(), values.data(), active.data()};
    fluid_sdf_attr_t at{g.n_leaves, ids.data(), velocity.data()};
    REQUIRE(g.n_leaves >= 2);
    struct Case { fluid_sdf_filter_t f; fluid_sdf_track_t t; };
    const Case cases[] = {{{1, 0, -3.0}, {3, 1, 0}}, {{1, 1, -3.0}, {3, 1, 0}}, {{1, 0, -4.0}, {1, 1, 0}}, {{2, 2, 4.0}, {2, 1, 0}}, {{1, 1, 0.0}, {8, 1, 0}},
                          {{1, 0, 1.0}, {3, 1, 0}}, {{4, 1, -0.25}, {1, 1, 0}}, {{1, 0, 0.0}, {3, 1, 0}}};
    int longer = 0, emptied = 0;
    for (const auto& cs : cases) {
        const int64_t k = fluid_sdf_filter_grown(&g, nullptr, &cs.f, &cs.t, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
        REQUIRE(k >= 0);
        REQUIRE(fluid_sdf_filter_grown(&g, &at, &cs.f, &cs.t, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == k);
        longer += k > g.n_leaves, emptied += k == 0;
        // exact capacities: a write past any of them is the sanitizer's to find
        std::vector<int32_t> oorg(3 * (size_t)k);
        std::vector<float> oval(512 * (size_t)k), ovel(1536 * (size_t)k);
        std::vector<uint64_t> oact(8 * (size_t)k);
        std::vector<uint32_t> oid(512 * (size_t)k);
        if (k == 0) {
            int32_t o1[3];
            float v1[512];
            uint64_t a1[8];
            REQUIRE(fluid_sdf_filter_grown(&g, nullptr, &cs.f, &cs.t, 0, o1, v1, a1, nullptr, nullptr) == 0);
            continue;
        }
        REQUIRE(fluid_sdf_filter_grown(&g, &at, &cs.f, &cs.t, k, oorg.data(), oval.data(), oact.data(), oid.data(), ovel.data()) == k);
        std::vector<int32_t> porg(3 * (size_t)k);
        std::vector<float> pval(512 * (size_t)k);
        std::vector<uint64_t> pact(8 * (size_t)k);
        REQUIRE(fluid_sdf_filter_grown(&g, nullptr, &cs.f, &cs.t, k, porg.data(), pval.data(), pact.data(), nullptr, nullptr) == k);
        REQUIRE(porg == oorg && pact == oact && memcmp(pval.data(), oval.data(), pval.size() * sizeof(float)) == 0);
        if (k > 1) REQUIRE(fluid_sdf_filter_grown(&g, &at, &cs.f, &cs.t, k - 1, oorg.data(), oval.data(), oact.data(), oid.data(), ovel.data()) == -FLUID_ERR_ARG);
        for (int64_t l = 0; l < k; ++l) {
            const int32_t* o = &oorg[3 * (size_t)l];
            for (int a = 0; a < 3; ++a) REQUIRE((o[a] & 7) == 0 && o[a] >= L0 && o[a] <= hi);
            if (l > 0) REQUIRE(std::lexicographical_compare(o - 3, o, o, o + 3));
            bool any = false;
            for (int off = 0; off < 512; ++off) {
                const int c[3] = {o[0] + (off >> 6), o[1] + ((off >> 3) & 7), o[2] + (off & 7)};
                const bool in = c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
                const bool act = (oact[8 * (size_t)l + (off >> 6)] >> (off & 63)) & 1ull;
                const float v = oval[512 * (size_t)l + off];
                const uint32_t id = oid[512 * (size_t)l + off];
                REQUIRE(in || !act);
                REQUIRE(act ? (v > -bg && v < bg) : (v == bg || v == -bg));
                REQUIRE(act == (id != FLUID_SDF_NO_ID));
                if (act) REQUIRE(given.count(id) == 1);
                else
                    for (int a = 0; a < 3; ++a) REQUIRE(ovel[1536 * (size_t)l + 512 * a + off] == 0.0f);
                any = any || (in && (act || v != bg));
            }
            REQUIRE(any);
        }
    }
    REQUIRE(longer >= 2 && emptied >= 1);
    // refusals: nothing is written
    const size_t cap = 64;
    std::vector<int32_t> oorg(3 * cap, 7);
    std::vector<float> oval(512 * cap, 7.0f), ovel(1536 * cap, 7.0f);
    std::vector<uint64_t> oact(8 * cap, 7);
    std::vector<uint32_t> oid(512 * cap, 7);
    auto untouched = [&]() {
        return std::all_of(oorg.begin(), oorg.end(), [](int32_t x) { return x == 7; }) && std::all_of(oval.begin(), oval.end(), [](float x) { return x == 7.0f; }) &&
               std::all_of(ovel.begin(), ovel.end(), [](float x) { return x == 7.0f; }) && std::all_of(oact.begin(), oact.end(), [](uint64_t x) { return x == 7; }) &&
               std::all_of(oid.begin(), oid.end(), [](uint32_t x) { return x == 7; });
    };
    const fluid_sdf_filter_t f{1, 0, -3.0}, far{1, 0, std::nextafter(4.0f, 5.0f)}, edge{1, 0, 4.0};
    const fluid_sdf_track_t t{3, 1, 0}, t0{0, 1, 0}, notrim{3, 0, 0}, t9{9, 1, 0}, scheme{3, 1, 1};
    auto call = [&](const fluid_sdf_attr_t* a, const fluid_sdf_filter_t* ff, const fluid_sdf_track_t* tt, int64_t c, uint32_t* i, float* ve) {
        return fluid_sdf_filter_grown(&g, a, ff, tt, c, oorg.data(), oval.data(), oact.data(), i, ve);
    };
    REQUIRE(call(&at, &f, &t0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &notrim, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &t9, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &scheme, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, nullptr, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, nullptr, &t, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &far, &t, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &t, cap, nullptr, ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &t, cap, oid.data(), nullptr) == -FLUID_ERR_ARG);
    REQUIRE(call(nullptr, &f, &t, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &t, 1, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, &f, &t, -1, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    fluid_sdf_attr_t wrong{g.n_leaves - 1, ids.data(), velocity.data()}, hollow{g.n_leaves, nullptr, velocity.data()};
    REQUIRE(call(&wrong, &f, &t, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&hollow, &f, &t, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_grown(&g, &at, &f, &t, cap, oorg.data(), values.data(), oact.data(), oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_grown(&g, &at, &f, &t, cap, oorg.data(), oval.data(), oact.data(), ids.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(untouched());
    REQUIRE(call(&at, &edge, &t, cap, oid.data(), ovel.data()) >= 0);
    fluid_sdf_grid_t e{n, 0, bg, R, w, nullptr, nullptr, nullptr};
    REQUIRE(fluid_sdf_filter_grown(&e, nullptr, &f, &t, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    printf("host sanitizer run (grow): ok\n");
    return 0;
}
