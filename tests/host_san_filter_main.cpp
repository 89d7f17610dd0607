// Stand-alone driver of the host level-set filter for the sanitizer build (tests/test_sdf_filter_host.py): a small built-in leaf
// list — a ball that straddles the corner where eight leaves meet, a second one cut by the grid's lo face, at n = 25, where the
// grid ends inside a leaf on both sides — goes through fluid_sdf_filter with every width, odd and even pass counts, the offset
// alone and the identity, and is compared with a plain dense restatement of the definition; then the refusals.
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

int main()
{
    const int n = 25, lo = -(n / 2), hi = lo + n - 1, L0 = lo & ~7;
    const float bg = 2.0f;
    const float centre[2][3] = {{-0.4f, -0.3f, -0.6f}, {(float)lo + 0.4f, 3.2f, 8.1f}};
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
    std::vector<float> dval((size_t)n * n * n, bg);
    std::vector<char> dact((size_t)n * n * n, 0);
    auto at = [&](int x, int y, int z) { return ((size_t)(x - lo) * n + (y - lo)) * n + (z - lo); };
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
                            const float e = std::sqrt((c[0] - p[0]) * (c[0] - p[0]) + (c[1] - p[1]) * (c[1] - p[1]) + (c[2] - p[2]) * (c[2] - p[2])) - 3.0f;
                            d = e < d ? e : d;
                        }
                    bool act = false;
                    if (d <= -bg) d = -bg;
                    else if (d < bg) act = true, m[off >> 6] |= 1ull << (off & 63);
                    v[off] = d;
                    listed = listed || d != bg;
                    if (in) dval[at(c[0], c[1], c[2])] = d, dact[at(c[0], c[1], c[2])] = act;
                }
                if (!listed) continue;
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
            }
    fluid_sdf_grid_t g{n, (int32_t)(origin.size() / 3), bg, 3.0f, 1.0f, origin.data(), values.data(), active.data()};
    REQUIRE(g.n_leaves >= 9);
    std::vector<float> out(values.size());
    const fluid_sdf_filter_t filters[] = {{1, 1, 0.0}, {1, 2, 0.0}, {2, 1, 0.0}, {3, 2, 0.5}, {4, 3, 0.0}, {1, 0, -0.25}, {1, 0, 0.0}, {4, 16, -1.0}};
    for (const auto& f : filters) {
        // the definition on the dense grid: +bg outside, axes x, z, y, Jacobi
        std::vector<float> cur = dval, nxt;
        const float frac = 1.0f / (float)(2 * f.width + 1);
        static const int axes[3] = {0, 2, 1};
        for (int k = 0; k < 3 * f.iterations; ++k) {
            nxt = cur;
            const int a = axes[k % 3];
            for (int x = lo; x <= hi; ++x)
                for (int y = lo; y <= hi; ++y)
                    for (int z = lo; z <= hi; ++z) {
                        if (!dact[at(x, y, z)]) continue;
                        float s = 0.0f;
                        for (int i = -f.width; i <= f.width; ++i) {
                            int c[3] = {x, y, z};
                            c[a] += i;
                            s = s + (c[a] < lo || c[a] > hi ? bg : cur[at(c[0], c[1], c[2])]);
                        }
                        nxt[at(x, y, z)] = s * frac;
                    }
            cur.swap(nxt);
        }
        const float off = (float)f.offset;
        if (off != 0.0f)
            for (size_t i = 0; i < cur.size(); ++i)
                if (dact[i]) cur[i] = cur[i] + off;
        std::fill(out.begin(), out.end(), 7.0f);
        REQUIRE(fluid_sdf_filter(&g, &f, out.data()) == FLUID_OK);
        bool moved = false;
        for (int l = 0; l < g.n_leaves; ++l)
            for (int o = 0; o < 512; ++o) {
                const int c[3] = {origin[3 * l] + (o >> 6), origin[3 * l + 1] + ((o >> 3) & 7), origin[3 * l + 2] + (o & 7)};
                const bool in = c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
                const float want = in ? cur[at(c[0], c[1], c[2])] : values[512 * (size_t)l + o];
                REQUIRE(memcmp(&want, &out[512 * (size_t)l + o], 4) == 0);
                moved = moved || memcmp(&values[512 * (size_t)l + o], &out[512 * (size_t)l + o], 4) != 0;
            }
        REQUIRE(moved == (f.iterations > 0 || off != 0.0f));
    }
    const fluid_sdf_filter_t ok{1, 1, 0.0};
    for (const fluid_sdf_filter_t& bad : {fluid_sdf_filter_t{0, 1, 0.0}, fluid_sdf_filter_t{5, 1, 0.0}, fluid_sdf_filter_t{1, -1, 0.0}, fluid_sdf_filter_t{1, 17, 0.0},
                                          fluid_sdf_filter_t{1, 1, std::numeric_limits<double>::quiet_NaN()}})
        REQUIRE(fluid_sdf_filter(&g, &bad, out.data()) == FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter(&g, &ok, nullptr) == FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter(&g, nullptr, out.data()) == FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter(&g, &ok, values.data()) == FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_filter(&g, &ok, values.data() + 512) == FLUID_ERR_ARG);
    fluid_sdf_grid_t none{n, 0, bg, 3.0f, 1.0f, nullptr, nullptr, nullptr};
    REQUIRE(fluid_sdf_filter(&none, &ok, nullptr) == FLUID_OK);
    std::swap(origin[0], origin[3]);   // (the first two leaves: no longer ascending)
    std::swap(origin[1], origin[4]);
    std::swap(origin[2], origin[5]);
    REQUIRE(fluid_sdf_filter(&g, &ok, out.data()) == FLUID_ERR_ARG);
    printf("host sanitizer run (filter): ok %d\n", (int)g.n_leaves);
    return 0;
}
