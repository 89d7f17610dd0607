// Stand-alone driver of the host HJWENO5 renormalisation for the sanitizer build (tests/test_sdf_weno_host.py): the built-in leaf
// list of host_san_track_main.cpp — a ball that straddles the corner where eight leaves meet, a second one cut by the grid's lo
// face, at n = 25, where the grid ends inside a leaf on both sides, with one leaf taken off the list (an unlisted neighbour in the
// middle of a band, read three planes deep) — goes through fluid_sdf_filter_tracked, fluid_sdf_filter_grown (with attributes) and
// fluid_sdf_flow (a median and a mean-curvature flow, tracked and grown) with scheme FLUID_SDF_TRACK_HJWENO5.  What the bytes are is
// tests/test_sdf_weno_host.py's business; here the reads and writes, the counts, the finiteness, that the scheme matters, that
// FIRST_BIAS after it gives what it gave before, and the refusals, none of which may write.
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
    const int n = 25, lo = -(n / 2), hi = lo + n - 1, L0 = lo & ~7;
    const float bg = 2.0f, R = 3.0f, w = 2.0f;
    const float centre[2][3] = {{-0.4f, -0.3f, -0.6f}, {(float)lo + 0.4f, 3.2f, 8.1f}};
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
    int seen = 0;
    for (int ox = L0; ox <= hi; ox += 8)
        for (int oy = L0; oy <= hi; oy += 8)
            for (int oz = L0; oz <= hi; oz += 8) {
                float v[512];
                uint64_t m[8] = {};
                bool listed = false;
                for (int off = 0; off < 512; ++off) {
                    const int c[3] = {ox + (off >> 6), oy + ((off >> 3) & 7), oz + (off & 7)};
                    float d = bg;
                    bool in = true;
                    for (int a = 0; a < 3; ++a) in = in && c[a] >= lo && c[a] <= hi;
                    if (in)
                        for (const auto& p : centre) {
                            const float e = std::sqrt((c[0] - p[0]) * (c[0] - p[0]) + (c[1] - p[1]) * (c[1] - p[1]) + (c[2] - p[2]) * (c[2] - p[2])) - R;
                            d = e < d ? e : d;
                        }
                    if (d <= -bg) d = -bg;
                    else if (d < bg) m[off >> 6] |= 1ull << (off & 63);
                    v[off] = d;
                    listed = listed || d != bg;
                }
                if (!listed || seen++ == 1) continue;   // the second listed leaf stays off the list: +bg to its neighbours
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
            }
    const fluid_sdf_grid_t g{n, (int32_t)(origin.size() / 3), bg, R, w, origin.data(), values.data(), active.data()};
    REQUIRE(g.n_leaves >= 8);
    const size_t nl = (size_t)g.n_leaves;
    std::vector<uint32_t> ids(512 * nl);
    std::vector<float> vel(1536 * nl);
    for (size_t i = 0; i < ids.size(); ++i) {
        const bool act = (active[8 * (i / 512) + ((i % 512) >> 6)] >> (i & 63)) & 1ull;
        ids[i] = act ? (uint32_t)(i % 977) : FLUID_SDF_NO_ID;
        for (int a = 0; a < 3; ++a) vel[1536 * (i / 512) + 512 * a + i % 512] = act ? 0.25f * (float)((i + a) % 13) : 0.0f;
    }
    const fluid_sdf_attr_t at{g.n_leaves, ids.data(), vel.data()};

    // ---- fluid_sdf_filter_tracked: both schemes, the first again afterwards
    struct Case { fluid_sdf_filter_t f; fluid_sdf_track_t t; };
    const Case cases[] = {{{1, 1, 0.0}, {3, 1, 4}}, {{1, 2, -0.25}, {3, 1, 4}}, {{1, 0, 0.6}, {2, 1, 4}}, {{2, 1, 0.0}, {1, 0, 4}}, {{1, 0, 2.0}, {8, 1, 4}}};
    std::vector<int32_t> oorg(3 * nl), okept(nl);
    std::vector<float> oval(512 * nl), first(512 * nl), again(512 * nl);
    std::vector<uint64_t> oact(8 * nl);
    int differs = 0;
    for (const auto& cs : cases) {
        fluid_sdf_track_t t0 = cs.t;
        t0.scheme = FLUID_SDF_TRACK_FIRST_BIAS;
        std::fill(first.begin(), first.end(), 7.0f);
        const int64_t k0 = fluid_sdf_filter_tracked(&g, &cs.f, &t0, g.n_leaves, oorg.data(), first.data(), oact.data(), okept.data());
        REQUIRE(k0 >= 0 && k0 <= g.n_leaves);
        const int64_t k = fluid_sdf_filter_tracked(&g, &cs.f, &cs.t, 0, nullptr, nullptr, nullptr, nullptr);   // the count alone
        REQUIRE(k >= 0 && k <= g.n_leaves);
        std::fill(oval.begin(), oval.end(), 7.0f);
        if (k > 0) REQUIRE(fluid_sdf_filter_tracked(&g, &cs.f, &cs.t, k - 1, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
        for (float x : oval) REQUIRE(x == 7.0f);
        REQUIRE(fluid_sdf_filter_tracked(&g, &cs.f, &cs.t, k, oorg.data(), oval.data(), oact.data(), okept.data()) == k);
        for (size_t i = 0; i < 512 * (size_t)k; ++i) REQUIRE(std::isfinite(oval[i]) && std::fabs(oval[i]) <= 3.0f * bg);
        for (int64_t i = 0; i < k; ++i) REQUIRE(okept[(size_t)i] >= 0 && okept[(size_t)i] < g.n_leaves && (i == 0 || okept[(size_t)i] > okept[(size_t)i - 1]));
        differs += k != k0 || memcmp(oval.data(), first.data(), 2048 * (size_t)k) != 0;
        std::fill(again.begin(), again.end(), 7.0f);
        REQUIRE(fluid_sdf_filter_tracked(&g, &cs.f, &t0, g.n_leaves, oorg.data(), again.data(), oact.data(), okept.data()) == k0);
        REQUIRE(memcmp(again.data(), first.data(), 2048 * nl) == 0);
    }
    REQUIRE(differs == (int)(sizeof(cases) / sizeof(cases[0])));   // the scheme is not ignored

    // ---- fluid_sdf_filter_grown with attributes: the band walks outwards by 1.5 voxels
    const fluid_sdf_filter_t grow_f{1, 1, -1.5};
    const fluid_sdf_track_t t4{3, 1, FLUID_SDF_TRACK_HJWENO5};
    const int64_t kg = fluid_sdf_filter_grown(&g, &at, &grow_f, &t4, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    REQUIRE(kg > 0);
    {
        std::vector<int32_t> go(3 * (size_t)kg);
        std::vector<float> gv(512 * (size_t)kg), gvel(1536 * (size_t)kg);
        std::vector<uint64_t> ga(8 * (size_t)kg);
        std::vector<uint32_t> gid(512 * (size_t)kg);
        REQUIRE(fluid_sdf_filter_grown(&g, &at, &grow_f, &t4, kg, go.data(), gv.data(), ga.data(), gid.data(), gvel.data()) == kg);
        for (size_t i = 0; i < gv.size(); ++i) {
            const bool act = (ga[8 * (i / 512) + ((i % 512) >> 6)] >> (i & 63)) & 1ull;
            REQUIRE(std::isfinite(gv[i]));
            const int32_t* o = &go[3 * (i / 512)];
            const int c[3] = {o[0] + (int)((i % 512) >> 6), o[1] + (int)(((i % 512) >> 3) & 7), o[2] + (int)(i & 7)};
            const bool in = c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
            if (in) REQUIRE(act == (gid[i] != FLUID_SDF_NO_ID));
        }
        REQUIRE(fluid_sdf_filter_grown(&g, &at, &grow_f, &t4, kg - 1, go.data(), gv.data(), ga.data(), gid.data(), gvel.data()) == -FLUID_ERR_ARG);
    }

    // ---- fluid_sdf_flow: a median and a mean-curvature flow, tracked and grown
    for (const int kind : {FLUID_SDF_FILTER_MEDIAN, FLUID_SDF_FILTER_MEAN_CURVATURE})
        for (const int grow : {0, 1}) {
            const fluid_sdf_filter_t ff{1, 2, 0.5};
            const int64_t kf = fluid_sdf_flow(&g, nullptr, kind, &ff, &t4, grow, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
            REQUIRE(kf > 0);
            std::vector<int32_t> fo(3 * (size_t)kf);
            std::vector<float> fv(512 * (size_t)kf);
            std::vector<uint64_t> fa(8 * (size_t)kf);
            REQUIRE(fluid_sdf_flow(&g, nullptr, kind, &ff, &t4, grow, kf, fo.data(), fv.data(), fa.data(), nullptr, nullptr) == kf);
            for (float x : fv) REQUIRE(std::isfinite(x));
        }

    // ---- the refusals: the schemes that are not built, for all three
    const fluid_sdf_filter_t ok{1, 1, 0.0};
    std::fill(oval.begin(), oval.end(), 7.0f);
    for (const int bad : {-1, 1, 2, 3, 5}) {
        const fluid_sdf_track_t tb{3, 1, bad};
        REQUIRE(fluid_sdf_filter_tracked(&g, &ok, &tb, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
        REQUIRE(fluid_sdf_filter_grown(&g, nullptr, &ok, &tb, g.n_leaves, oorg.data(), oval.data(), oact.data(), nullptr, nullptr) == -FLUID_ERR_ARG);
        REQUIRE(fluid_sdf_flow(&g, nullptr, FLUID_SDF_FILTER_MEDIAN, &ok, &tb, 0, g.n_leaves, oorg.data(), oval.data(), oact.data(), nullptr, nullptr) == -FLUID_ERR_ARG);
    }
    const fluid_sdf_filter_t far{1, 1, 2.5};   // |off| > bg
    REQUIRE(fluid_sdf_filter_tracked(&g, &far, &t4, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    const fluid_sdf_track_t t9{9, 1, FLUID_SDF_TRACK_HJWENO5}, notrim{3, 0, FLUID_SDF_TRACK_HJWENO5};
    REQUIRE(fluid_sdf_filter_tracked(&g, &ok, &t9, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_grown(&g, nullptr, &ok, &notrim, g.n_leaves, oorg.data(), oval.data(), oact.data(), nullptr, nullptr) == -FLUID_ERR_ARG);
    for (float x : oval) REQUIRE(x == 7.0f);
    const fluid_sdf_grid_t none{n, 0, bg, R, w, nullptr, nullptr, nullptr};
    REQUIRE(fluid_sdf_filter_tracked(&none, &ok, &t4, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    printf("host sanitizer run (weno): ok %d\n", (int)g.n_leaves);
    return 0;
}
