// Stand-alone driver of the host tracked level-set filter for the sanitizer build (tests/test_sdf_track_host.py): the built-in leaf
// list of host_san_filter_main.cpp — a ball that straddles the corner where eight leaves meet, a second one cut by the grid's lo
// face, at n = 25, where the grid ends inside a leaf on both sides — with one of its leaves taken off the list (an unlisted
// neighbour in the middle of a band) goes through fluid_sdf_filter_tracked and is compared with a plain dense restatement of the
// definition; then the count-only mode, kept, and the refusals, none of which may write.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "fluid_hip.h"

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);  \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static float mx(float a, float b) { return a < b ? b : a; }
static float mn(float a, float b) { return b < a ? b : a; }

int main()
{
    const int n = 25, lo = -(n / 2), hi = lo + n - 1, L0 = lo & ~7;
    const float bg = 2.0f, R = 3.0f, w = 2.0f, dx = 1.0f;
    const float centre[2][3] = {{-0.4f, -0.3f, -0.6f}, {(float)lo + 0.4f, 3.2f, 8.1f}};
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
    std::vector<float> dval((size_t)n * n * n, bg);
    std::vector<char> dact((size_t)n * n * n, 0);
    auto at = [&](int x, int y, int z) { return ((size_t)(x - lo) * n + (y - lo)) * n + (z - lo); };
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
                for (int off = 0; off < 512; ++off) {
                    const int c[3] = {ox + (off >> 6), oy + ((off >> 3) & 7), oz + (off & 7)};
                    if (c[0] < lo || c[0] > hi || c[1] < lo || c[1] > hi || c[2] < lo || c[2] > hi) continue;
                    dval[at(c[0], c[1], c[2])] = v[off], dact[at(c[0], c[1], c[2])] = (m[off >> 6] >> (off & 63)) & 1;
                }
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
            }
    fluid_sdf_grid_t g{n, (int32_t)(origin.size() / 3), bg, R, w, origin.data(), values.data(), active.data()};
    REQUIRE(g.n_leaves >= 8);
    const size_t nl = (size_t)g.n_leaves;
    std::vector<int32_t> oorg(3 * nl), okept(nl);
    std::vector<float> oval(512 * nl);
    std::vector<uint64_t> oact(8 * nl);
    struct Case { fluid_sdf_filter_t f; fluid_sdf_track_t t; };
    const Case cases[] = {{{1, 1, 0.0}, {3, 1, 0}}, {{1, 2, 0.0}, {3, 1, 0}}, {{2, 1, 0.0}, {1, 0, 0}}, {{1, 0, -0.25}, {3, 1, 0}}, {{1, 0, 0.6}, {2, 1, 0}},
                          {{4, 3, 0.0}, {2, 1, 0}}, {{1, 0, 0.0}, {8, 1, 0}}, {{1, 0, 2.0}, {0, 1, 0}}};
    const float dt = dx * 0.3f, inv = 1.0f / dx;
    int unlisted_some = 0;
    for (const auto& cs : cases) {
        std::vector<float> cur = dval, nxt;
        std::vector<char> act = dact;
        auto rd = [&](const std::vector<float>& a, int x, int y, int z) { return x < lo || x > hi || y < lo || y > hi || z < lo || z > hi ? bg : a[at(x, y, z)]; };
        auto track = [&]() {
            for (int i = 0; i < cs.t.normalize; ++i) {
                nxt = cur;
                for (int x = lo; x <= hi; ++x)
                    for (int y = lo; y <= hi; ++y)
                        for (int z = lo; z <= hi; ++z) {
                            if (!act[at(x, y, z)]) continue;
                            const float p = cur[at(x, y, z)];
                            const bool out = p > 0.0f;
                            float G = 0.0f;
                            for (int a = 0; a < 3; ++a) {
                                const int e[3] = {a == 0, a == 1, a == 2};
                                const float dm = p - rd(cur, x - e[0], y - e[1], z - e[2]), dp = rd(cur, x + e[0], y + e[1], z + e[2]) - p;
                                const float A = out ? mx(dm, 0.0f) : mn(dm, 0.0f), B = out ? mn(dp, 0.0f) : mx(dp, 0.0f);
                                const float t = mx(A * A, B * B);
                                G = a == 0 ? t : G + t;
                            }
                            const float S = p / (std::sqrt(p * p + G) + 1e-8f);
                            nxt[at(x, y, z)] = p - (dt * S) * (std::sqrt(G) * inv - 1.0f);
                        }
                cur.swap(nxt);
            }
            if (cs.t.trim)
                for (size_t i = 0; i < cur.size(); ++i)
                    if (act[i] && (cur[i] <= -bg || cur[i] >= bg)) cur[i] = cur[i] <= -bg ? -bg : bg, act[i] = 0;
        };
        const float frac = 1.0f / (float)(2 * cs.f.width + 1);
        static const int axes[3] = {0, 2, 1};
        for (int k = 0; k < 3 * cs.f.iterations; ++k) {
            nxt = cur;
            const int a = axes[k % 3];
            for (int x = lo; x <= hi; ++x)
                for (int y = lo; y <= hi; ++y)
                    for (int z = lo; z <= hi; ++z) {
                        if (!act[at(x, y, z)]) continue;
                        float s = 0.0f;
                        for (int i = -cs.f.width; i <= cs.f.width; ++i) {
                            int c[3] = {x, y, z};
                            c[a] += i;
                            s = s + rd(cur, c[0], c[1], c[2]);
                        }
                        nxt[at(x, y, z)] = s * frac;
                    }
            cur.swap(nxt);
            if (k % 3 == 2) track();
        }
        const float off = (float)cs.f.offset, CFL = 0.5f * dx, a = std::fabs(off);
        float d = 0.0f;
        while (a - d > 0.001f * CFL) {
            const float delta = a - d < CFL ? a - d : CFL;
            d = d + delta;
            for (size_t i = 0; i < cur.size(); ++i)
                if (act[i]) cur[i] = cur[i] + std::copysign(delta, off);
            track();
        }
        const int64_t k = fluid_sdf_filter_tracked(&g, &cs.f, &cs.t, 0, nullptr, nullptr, nullptr, nullptr);   // the count alone
        REQUIRE(k >= 0 && k <= g.n_leaves);
        std::fill(oval.begin(), oval.end(), 7.0f);
        if (k > 0) REQUIRE(fluid_sdf_filter_tracked(&g, &cs.f, &cs.t, k - 1, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
        for (float x : oval) REQUIRE(x == 7.0f);
        REQUIRE(fluid_sdf_filter_tracked(&g, &cs.f, &cs.t, k, oorg.data(), oval.data(), oact.data(), okept.data()) == k);
        unlisted_some += k < g.n_leaves;
        // every listed leaf of the input: kept with the dense result's in-grid voxels, or dropped and all inactive +bg there
        int64_t i = 0;
        for (int l = 0; l < g.n_leaves; ++l) {
            const bool is_kept = i < k && okept[(size_t)i] == l;
            if (is_kept) REQUIRE(memcmp(&oorg[3 * (size_t)i], &origin[3 * (size_t)l], 12) == 0);
            for (int o = 0; o < 512; ++o) {
                const int c[3] = {origin[3 * l] + (o >> 6), origin[3 * l + 1] + ((o >> 3) & 7), origin[3 * l + 2] + (o & 7)};
                const bool in = c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
                if (!is_kept) {
                    if (in) REQUIRE(!act[at(c[0], c[1], c[2])] && cur[at(c[0], c[1], c[2])] == bg);
                    continue;
                }
                const float want = in ? cur[at(c[0], c[1], c[2])] : values[512 * (size_t)l + o];
                const bool wact = in ? act[at(c[0], c[1], c[2])] != 0 : ((active[8 * (size_t)l + (o >> 6)] >> (o & 63)) & 1) != 0;
                REQUIRE(memcmp(&want, &oval[512 * (size_t)i + o], 4) == 0);
                REQUIRE(wact == (((oact[8 * (size_t)i + (o >> 6)] >> (o & 63)) & 1) != 0));
            }
            i += is_kept;
        }
        REQUIRE(i == k);
    }
    REQUIRE(unlisted_some >= 1);   // (the last case shrinks the liquid by the whole band: the leaves that held the outer band alone leave the list)
    const fluid_sdf_filter_t ok{1, 1, 0.0};
    const fluid_sdf_track_t tk{3, 1, 0};
    std::fill(oval.begin(), oval.end(), 7.0f);
    // t == NULL: fluid_sdf_filter plus the copy of masks and origins
    std::vector<float> plain(512 * nl);
    REQUIRE(fluid_sdf_filter(&g, &ok, plain.data()) == FLUID_OK);
    REQUIRE(fluid_sdf_filter_tracked(&g, &ok, nullptr, g.n_leaves, oorg.data(), oval.data(), oact.data(), nullptr) == g.n_leaves);
    REQUIRE(memcmp(plain.data(), oval.data(), 2048 * nl) == 0 && memcmp(oorg.data(), origin.data(), 12 * nl) == 0 && memcmp(oact.data(), active.data(), 64 * nl) == 0);
    std::fill(oval.begin(), oval.end(), 7.0f);
    for (const fluid_sdf_track_t& bad : {fluid_sdf_track_t{-1, 1, 0}, fluid_sdf_track_t{9, 1, 0}, fluid_sdf_track_t{3, 2, 0}, fluid_sdf_track_t{3, 1, 1}})
        REQUIRE(fluid_sdf_filter_tracked(&g, &ok, &bad, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    const fluid_sdf_filter_t far{1, 1, 2.5};   // |off| > bg
    REQUIRE(fluid_sdf_filter_tracked(&g, &far, &tk, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_tracked(&g, &far, nullptr, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == g.n_leaves);   // untracked: allowed
    std::fill(oval.begin(), oval.end(), 7.0f);
    const fluid_sdf_filter_t badf{5, 1, 0.0};
    REQUIRE(fluid_sdf_filter_tracked(&g, &badf, &tk, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_tracked(&g, nullptr, &tk, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_tracked(nullptr, &ok, &tk, g.n_leaves, oorg.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_tracked(&g, &ok, &tk, g.n_leaves, oorg.data(), nullptr, oact.data(), okept.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter_tracked(&g, &ok, &tk, g.n_leaves, oorg.data(), values.data() + 512, oact.data(), okept.data()) == -FLUID_ERR_ARG);   // overlap
    REQUIRE(fluid_sdf_filter_tracked(&g, &ok, &tk, g.n_leaves, origin.data(), oval.data(), oact.data(), okept.data()) == -FLUID_ERR_ARG);
    for (float x : oval) REQUIRE(x == 7.0f);
    fluid_sdf_grid_t none{n, 0, bg, R, w, nullptr, nullptr, nullptr};
    REQUIRE(fluid_sdf_filter_tracked(&none, &ok, &tk, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    printf("host sanitizer run (track): ok %d\n", (int)g.n_leaves);
    return 0;
}
