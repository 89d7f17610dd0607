// Stand-alone driver of the host mesher and the PLY writer for the sanitizer build (tests/test_mesh_host.py): a small built-in
// leaf list — a ball that straddles the corner where eight leaves meet, a second one cut by the grid's lo face, at n = 25, where
// the grid ends inside a leaf on both sides — goes through fluid_sdf_mesh (counts only, caps too small, the arrays) and
// fluid_write_ply_mesh (a file, an unwritable path).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fluid_hip.h"

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);  \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int n = 25, lo = -(n / 2), hi = lo + n - 1, L0 = lo & ~7;
    const float bg = 2.0f;
    const float centre[2][3] = {{-0.4f, -0.3f, -0.6f}, {(float)lo + 0.4f, 3.2f, 8.1f}};
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
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
                    if (d <= -bg) d = -bg;
                    else if (d < bg) m[off >> 6] |= 1ull << (off & 63);
                    v[off] = d;
                    listed = listed || d != bg;
                }
                if (!listed) continue;
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
            }
    fluid_sdf_grid_t g{n, (int32_t)(origin.size() / 3), bg, 3.0f, 1.0f, origin.data(), values.data(), active.data()};
    REQUIRE(g.n_leaves >= 9);
    int64_t nq = -1;
    const int64_t nv = fluid_sdf_mesh(&g, 0, 0, nullptr, nullptr, &nq);
    REQUIRE(nv > 100 && nq > 100);
    std::vector<float> vert((size_t)3 * nv);
    std::vector<uint32_t> quad((size_t)4 * nq);
    REQUIRE(fluid_sdf_mesh(&g, nv - 1, nq, vert.data(), quad.data(), nullptr) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_mesh(&g, nv, nq - 1, vert.data(), quad.data(), nullptr) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_mesh(&g, nv, nq, vert.data(), nullptr, nullptr) == -FLUID_ERR_ARG);
    int64_t nq2 = -1;
    REQUIRE(fluid_sdf_mesh(&g, nv, nq, vert.data(), quad.data(), &nq2) == nv && nq2 == nq);
    for (uint32_t i : quad) REQUIRE((int64_t)i < nv);
    for (float c : vert) REQUIRE(c >= (float)lo && c <= (float)hi);
    std::swap(origin[0], origin[3]);   // (x of the first two leaves: no longer ascending, or no longer a list at all)
    std::swap(origin[1], origin[4]);
    std::swap(origin[2], origin[5]);
    REQUIRE(fluid_sdf_mesh(&g, 0, 0, nullptr, nullptr, nullptr) == -FLUID_ERR_ARG);
    fluid_sdf_grid_t none{n, 0, bg, 3.0f, 1.0f, nullptr, nullptr, nullptr};
    REQUIRE(fluid_sdf_mesh(&none, 0, 0, nullptr, nullptr, &nq2) == 0 && nq2 == 0);

    const fluid_mesh_t m{n, nv, nq, 3.0f, 1.0f, bg, vert.data(), quad.data()};
    const std::string path = dir + "/san_mesh.ply";
    REQUIRE(fluid_write_ply_mesh(path.c_str(), &m, 0.5f) == FLUID_OK);
    FILE* f = fopen(path.c_str(), "rb");
    REQUIRE(f != nullptr);
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fclose(f);
    REQUIRE(size > 12 * nv + 17 * nq && size < 12 * nv + 17 * nq + 300);
    REQUIRE(fluid_write_ply_mesh((dir + "/no_such_dir/m.ply").c_str(), &m, 0.5f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh(path.c_str(), &m, 0.0f) == FLUID_ERR_ARG);
    const fluid_mesh_t empty{n, 0, 0, 3.0f, 1.0f, bg, nullptr, nullptr};
    REQUIRE(fluid_write_ply_mesh((dir + "/san_empty.ply").c_str(), &empty, 1.0f) == FLUID_OK);
    printf("host sanitizer run (mesh): ok %lld %lld\n", (long long)nv, (long long)nq);
    return 0;
}
