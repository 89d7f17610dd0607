// Stand-alone driver of the host level-set flows for the sanitizer build (tests/test_sdf_flow_host.py): two balls at n = 20, where the
// grid [-10, 9] ends inside a leaf on both sides — one around the corner (0, 0, 0) where eight leaves meet, so that edge and corner
// leaves feed the tiles, one cut by the grid's lo face — with an id and a velocity per active voxel go through fluid_sdf_flow for
// every kind and width, untracked, tracked and grown, with and without attributes.  What the definition promises is checked on every
// result (the bytes themselves are pinned by the Python tests): ascending origins on the 8-grid, finite values, inactive voxels at
// +-bg, nothing active outside the grid, active <=> has an id; untracked the list and the masks are the input's; then the count-only
// form, exact capacities, and the refusals, none of which may write.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    const float centre[2][3] = {{0.2f, 0.1f, 0.3f}, {(float)lo + 0.4f, -3.2f, 2.1f}};
    std::vector<int32_t> origin;
    std::vector<float> values, velocity;
    std::vector<uint64_t> active;
    std::vector<uint32_t> ids;
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
    REQUIRE(g.n_leaves >= 9);   // the eight leaves around the corner and the ball at the lo face
    struct Kind { int32_t kind, width; };
    const Kind kinds[] = {{FLUID_SDF_FILTER_BOX, 2}, {FLUID_SDF_FILTER_MEDIAN, 1}, {FLUID_SDF_FILTER_MEDIAN, 2}, {FLUID_SDF_FILTER_LAPLACIAN, 1},
                          {FLUID_SDF_FILTER_MEAN_CURVATURE, 1}};
    struct Form { bool tracked; fluid_sdf_track_t t; int32_t grow; double offset; };
    const Form forms[] = {{false, {0, 0, 0}, 0, 0.0}, {false, {0, 0, 0}, 0, -0.25}, {true, {3, 1, 0}, 0, 0.6}, {true, {2, 0, 0}, 0, 0.0}, {true, {3, 1, 0}, 1, -1.0},
                          {true, {1, 1, 0}, 1, 3.0}};
    for (const Kind& kd : kinds)
        for (const Form& fm : forms)
            for (int K = 0; K <= 3; K += 3) {
                const fluid_sdf_filter_t f{kd.width, K, fm.offset};
                const fluid_sdf_track_t* t = fm.tracked ? &fm.t : nullptr;
                const int64_t k = fluid_sdf_flow(&g, nullptr, kd.kind, &f, t, fm.grow, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
                REQUIRE(k >= 0);
                REQUIRE(fluid_sdf_flow(&g, &at, kd.kind, &f, t, fm.grow, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == k);
                if (!fm.tracked) REQUIRE(k == g.n_leaves);
                // exact capacities: a write past any of them is the sanitizer's to find
                std::vector<int32_t> oorg(3 * (size_t)k), porg(3 * (size_t)k);
                std::vector<float> oval(512 * (size_t)k), ovel(1536 * (size_t)k), pval(512 * (size_t)k);
                std::vector<uint64_t> oact(8 * (size_t)k), pact(8 * (size_t)k);
                std::vector<uint32_t> oid(512 * (size_t)k);
                if (k == 0) continue;
                REQUIRE(fluid_sdf_flow(&g, &at, kd.kind, &f, t, fm.grow, k, oorg.data(), oval.data(), oact.data(), oid.data(), ovel.data()) == k);
                REQUIRE(fluid_sdf_flow(&g, nullptr, kd.kind, &f, t, fm.grow, k, porg.data(), pval.data(), pact.data(), nullptr, nullptr) == k);
                REQUIRE(porg == oorg && pact == oact && memcmp(pval.data(), oval.data(), pval.size() * sizeof(float)) == 0);
                if (k > 1)
                    REQUIRE(fluid_sdf_flow(&g, &at, kd.kind, &f, t, fm.grow, k - 1, oorg.data(), oval.data(), oact.data(), oid.data(), ovel.data()) == -FLUID_ERR_ARG);
                if (!fm.tracked) REQUIRE(oorg == origin && oact == active && oid == ids && memcmp(ovel.data(), velocity.data(), ovel.size() * sizeof(float)) == 0);
                const bool trimmed = fm.tracked && fm.t.trim;
                for (int64_t l = 0; l < k; ++l) {
                    const int32_t* o = &oorg[3 * (size_t)l];
                    for (int a = 0; a < 3; ++a) REQUIRE((o[a] & 7) == 0 && o[a] >= L0 && o[a] <= hi);
                    if (l > 0) REQUIRE(std::lexicographical_compare(o - 3, o, o, o + 3));
                    for (int off = 0; off < 512; ++off) {
                        const int c[3] = {o[0] + (off >> 6), o[1] + ((off >> 3) & 7), o[2] + (off & 7)};
                        const bool in = c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
                        const bool act = (oact[8 * (size_t)l + (off >> 6)] >> (off & 63)) & 1ull;
                        const float v = oval[512 * (size_t)l + off];
                        REQUIRE(std::isfinite(v));
                        REQUIRE(in || !act);
                        if (!act) REQUIRE(v == bg || v == -bg);
                        if (act && trimmed) REQUIRE(v > -bg && v < bg);
                        REQUIRE(act == (oid[512 * (size_t)l + off] != FLUID_SDF_NO_ID));
                    }
                }
            }
    // kind = BOX is the three older functions
    {
        const fluid_sdf_filter_t f{1, 1, -0.5};
        const fluid_sdf_track_t t{3, 1, 0};
        const size_t nl = (size_t)g.n_leaves;
        std::vector<float> a(512 * nl), b(512 * nl);
        std::vector<int32_t> oa(3 * nl);
        std::vector<uint64_t> ma(8 * nl);
        REQUIRE(fluid_sdf_filter(&g, &f, a.data()) == FLUID_OK);
        REQUIRE(fluid_sdf_flow(&g, nullptr, FLUID_SDF_FILTER_BOX, &f, nullptr, 0, (int64_t)nl, oa.data(), b.data(), ma.data(), nullptr, nullptr) == (int64_t)nl);
        REQUIRE(memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0 && oa == origin && ma == active);
        const int64_t k = fluid_sdf_filter_tracked(&g, &f, &t, 0, nullptr, nullptr, nullptr, nullptr);
        REQUIRE(k > 0 && fluid_sdf_flow(&g, nullptr, FLUID_SDF_FILTER_BOX, &f, &t, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == k);
        std::vector<float> va(512 * (size_t)k), vb(512 * (size_t)k);
        std::vector<int32_t> ob(3 * (size_t)k), oc(3 * (size_t)k);
        std::vector<uint64_t> mb(8 * (size_t)k), mc(8 * (size_t)k);
        REQUIRE(fluid_sdf_filter_tracked(&g, &f, &t, k, ob.data(), va.data(), mb.data(), nullptr) == k);
        REQUIRE(fluid_sdf_flow(&g, nullptr, FLUID_SDF_FILTER_BOX, &f, &t, 0, k, oc.data(), vb.data(), mc.data(), nullptr, nullptr) == k);
        REQUIRE(ob == oc && mb == mc && memcmp(va.data(), vb.data(), va.size() * sizeof(float)) == 0);
    }
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
    const fluid_sdf_filter_t f1{1, 1, 0.0}, f2{2, 1, 0.0}, f3{3, 1, 0.0}, far{1, 1, std::nextafter(4.0f, 5.0f)}, deep{1, 1, std::nextafter(2.0f, 3.0f)};
    const fluid_sdf_track_t t{3, 1, 0}, notrim{3, 0, 0}, t9{9, 1, 0};
    auto call = [&](const fluid_sdf_attr_t* a, int32_t kind, const fluid_sdf_filter_t* ff, const fluid_sdf_track_t* tt, int32_t grow, int64_t c, uint32_t* i, float* ve) {
        return fluid_sdf_flow(&g, a, kind, ff, tt, grow, c, oorg.data(), oval.data(), oact.data(), i, ve);
    };
    REQUIRE(call(&at, -1, &f1, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, 4, &f1, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f3, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_LAPLACIAN, &f2, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEAN_CURVATURE, &f2, nullptr, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 2, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, &notrim, 1, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, nullptr, 1, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, &t9, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, nullptr, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &far, &t, 1, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &deep, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, cap, nullptr, ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(nullptr, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, 1, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, nullptr, 0, g.n_leaves - 1, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(call(&at, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, -1, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    fluid_sdf_attr_t wrong{g.n_leaves - 1, ids.data(), velocity.data()};
    REQUIRE(call(&wrong, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, cap, oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_flow(&g, &at, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, cap, oorg.data(), values.data(), oact.data(), oid.data(), ovel.data()) == -FLUID_ERR_ARG);
    fluid_sdf_grid_t nodx = g;
    nodx.half_width = 0.0f;   // no dx to be had: refused where dx is read, taken where it is not
    REQUIRE(fluid_sdf_flow(&nodx, nullptr, FLUID_SDF_FILTER_LAPLACIAN, &f1, nullptr, 0, cap, oorg.data(), oval.data(), oact.data(), nullptr, nullptr) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_flow(&nodx, nullptr, FLUID_SDF_FILTER_MEDIAN, &f1, &t, 0, cap, oorg.data(), oval.data(), oact.data(), nullptr, nullptr) == -FLUID_ERR_ARG);
    REQUIRE(untouched());
    REQUIRE(fluid_sdf_flow(&nodx, nullptr, FLUID_SDF_FILTER_MEDIAN, &f1, nullptr, 0, cap, oorg.data(), oval.data(), oact.data(), nullptr, nullptr) == g.n_leaves);
    fluid_sdf_grid_t e{n, 0, bg, R, w, nullptr, nullptr, nullptr};
    REQUIRE(fluid_sdf_flow(&e, nullptr, FLUID_SDF_FILTER_MEAN_CURVATURE, &f1, &t, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    printf("host sanitizer run (flow): ok\n");
    return 0;
}
