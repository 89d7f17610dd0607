// Stand-alone driver of the attribute host code for the sanitizer build (tests/test_attr_host.py): the small built-in leaf list of
// host_san_mesh_main.cpp — a ball that straddles the corner where eight leaves meet, a second one cut by the grid's lo face, at
// n = 25, where the grid ends inside a leaf on both sides — with an id and a velocity per active voxel, and one leaf whose mask is
// cleared by hand so that edges with one and with no active end occur.  It goes through fluid_sdf_mesh_attr (count only, a cap too
// small, attributes of another list, the array), fluid_sdf_attr_to_dense (both arrays, one, none, a bad list) and
// fluid_write_ply_mesh_attr (a file, a count mismatch, an unwritable path, an empty mesh).
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
    std::vector<float> values, vel;
    std::vector<uint64_t> active;
    std::vector<uint32_t> id;
    for (int ox = L0; ox <= hi; ox += 8)
        for (int oy = L0; oy <= hi; oy += 8)
            for (int oz = L0; oz <= hi; oz += 8) {
                float v[512], a[3][512];
                uint32_t who[512];
                uint64_t m[8] = {};
                bool listed = false;
                for (int off = 0; off < 512; ++off) {
                    const int c[3] = {ox + (off >> 6), oy + ((off >> 3) & 7), oz + (off & 7)};
                    float d = bg;
                    int nearest = 0;
                    bool in = true;
                    for (int k = 0; k < 3; ++k) in = in && c[k] >= lo && c[k] <= hi;
                    if (in)
                        for (int q = 0; q < 2; ++q) {
                            const float* p = centre[q];
                            const float e = std::sqrt((c[0] - p[0]) * (c[0] - p[0]) + (c[1] - p[1]) * (c[1] - p[1]) + (c[2] - p[2]) * (c[2] - p[2])) - 3.0f;
                            if (e < d) d = e, nearest = q;
                        }
                    bool act = false;
                    if (d <= -bg) d = -bg;
                    else if (d < bg) act = true;
                    if (act) m[off >> 6] |= 1ull << (off & 63);
                    v[off] = d;
                    who[off] = act ? (uint32_t)nearest : FLUID_SDF_NO_ID;
                    for (int k = 0; k < 3; ++k) a[k][off] = act ? 0.25f * (float)c[k] + (float)nearest : 0.0f;
                    listed = listed || d != bg;
                }
                if (!listed) continue;
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
                id.insert(id.end(), who, who + 512);
                for (int k = 0; k < 3; ++k) vel.insert(vel.end(), a[k], a[k] + 512);
            }
    fluid_sdf_grid_t g{n, (int32_t)(origin.size() / 3), bg, 3.0f, 1.0f, origin.data(), values.data(), active.data()};
    REQUIRE(g.n_leaves >= 9);
    for (int k = 0; k < 8; ++k) active[8 * 4 + k] = 0;   // the fifth leaf: values stay, nothing is active (a hand-made list)
    fluid_sdf_attr_t at{g.n_leaves, id.data(), vel.data()};

    int64_t nq = -1;
    const int64_t nv = fluid_sdf_mesh(&g, 0, 0, nullptr, nullptr, &nq);
    REQUIRE(nv > 100 && nq > 100);
    REQUIRE(fluid_sdf_mesh_attr(&g, &at, 0, nullptr) == nv);
    std::vector<float> vv((size_t)3 * nv, 7.0f);
    REQUIRE(fluid_sdf_mesh_attr(&g, &at, nv - 1, vv.data()) == -FLUID_ERR_ARG);
    const fluid_sdf_attr_t other{g.n_leaves - 1, id.data(), vel.data()}, no_id{g.n_leaves, nullptr, vel.data()};
    REQUIRE(fluid_sdf_mesh_attr(&g, &other, nv, vv.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_mesh_attr(&g, &no_id, nv, vv.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_mesh_attr(&g, nullptr, nv, vv.data()) == -FLUID_ERR_ARG);
    for (float c : vv) REQUIRE(c == 7.0f);   // nothing written
    REQUIRE(fluid_sdf_mesh_attr(&g, &at, nv, vv.data()) == nv);
    for (float c : vv) REQUIRE(std::isfinite(c) && std::fabs(c) <= 0.25f * 13.0f + 1.0f);

    const size_t n3 = (size_t)n * n * n;
    std::vector<uint32_t> did(n3);
    std::vector<float> dvel(3 * n3);
    REQUIRE(fluid_sdf_attr_to_dense(&g, &at, did.data(), dvel.data()) == FLUID_OK);
    size_t owned = 0;
    for (uint32_t i : did) owned += i != FLUID_SDF_NO_ID;
    REQUIRE(owned > 100);
    REQUIRE(fluid_sdf_attr_to_dense(&g, &at, did.data(), nullptr) == FLUID_OK);
    REQUIRE(fluid_sdf_attr_to_dense(&g, &at, nullptr, nullptr) == FLUID_OK);
    REQUIRE(fluid_sdf_attr_to_dense(&g, &other, did.data(), dvel.data()) == FLUID_ERR_ARG);

    std::vector<float> vert((size_t)3 * nv);
    std::vector<uint32_t> quad((size_t)4 * nq);
    REQUIRE(fluid_sdf_mesh(&g, nv, nq, vert.data(), quad.data(), nullptr) == nv);
    const fluid_mesh_t m{n, nv, nq, 3.0f, 1.0f, bg, vert.data(), quad.data()};
    const fluid_mesh_attr_t ma{nv, vv.data()}, fewer{nv - 1, vv.data()}, none{nv, nullptr};
    const std::string path = dir + "/san_attr.ply";
    REQUIRE(fluid_write_ply_mesh_attr(path.c_str(), &m, &fewer, 0.5f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_attr(path.c_str(), &m, &none, 0.5f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_attr(path.c_str(), &m, &ma, 0.0f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_attr(path.c_str(), &m, &ma, 0.5f, NAN) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_attr((dir + "/no_such_dir/m.ply").c_str(), &m, &ma, 0.5f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_attr(path.c_str(), &m, &ma, 0.5f, 2.0f) == FLUID_OK);
    FILE* f = fopen(path.c_str(), "rb");
    REQUIRE(f != nullptr);
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fclose(f);
    REQUIRE(size > 24 * nv + 17 * nq && size < 24 * nv + 17 * nq + 400);
    const fluid_mesh_t empty{n, 0, 0, 3.0f, 1.0f, bg, nullptr, nullptr};
    const fluid_mesh_attr_t empty_attr{0, nullptr};
    REQUIRE(fluid_write_ply_mesh_attr((dir + "/san_attr_empty.ply").c_str(), &empty, &empty_attr, 1.0f, 1.0f) == FLUID_OK);

    std::swap(origin[0], origin[3]);   // (no longer ascending)
    std::swap(origin[1], origin[4]);
    std::swap(origin[2], origin[5]);
    REQUIRE(fluid_sdf_mesh_attr(&g, &at, 0, nullptr) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_attr_to_dense(&g, &at, did.data(), dvel.data()) == FLUID_ERR_ARG);
    printf("host sanitizer run (attr): ok %lld %lld\n", (long long)nv, (long long)nq);
    return 0;
}
