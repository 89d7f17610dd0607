// Stand-alone driver of the normals-and-triangles host code for the sanitizer build (tests/test_mesh_normals_host.py): the small
// built-in leaf list of tests/attr_san_main.cpp — a ball that straddles the corner where eight leaves meet, a second one cut by the
// grid's lo face, at n = 25, where the grid ends inside a leaf on both sides — with one voxel just outside the surface set to NaN
// by hand.  It goes through fluid_sdf_mesh_normals (count only, a cap too small, the array, a bad list), fluid_mesh_triangles
// (count only, a cap too small, the array, an entry beyond the vertices, the empty mesh) and fluid_write_ply_mesh_ex (every
// combination of parts, a triangle count that is not twice the quad count, a triangle entry beyond the vertices, an unwritable path,
// an empty mesh).
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

static long file_size(const std::string& p)
{
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return -1;
    fseek(f, 0, SEEK_END);
    const long s = ftell(f);
    fclose(f);
    return s;
}

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
                    for (int k = 0; k < 3; ++k) in = in && c[k] >= lo && c[k] <= hi;
                    if (in)
                        for (int q = 0; q < 2; ++q) {
                            const float* p = centre[q];
                            const float e = std::sqrt((c[0] - p[0]) * (c[0] - p[0]) + (c[1] - p[1]) * (c[1] - p[1]) + (c[2] - p[2]) * (c[2] - p[2])) - 3.0f;
                            if (e < d) d = e;
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
    size_t just_outside = 0;
    while (just_outside < values.size() && !(values[just_outside] > 0.0f && values[just_outside] < 0.3f)) ++just_outside;
    REQUIRE(just_outside < values.size());
    values[just_outside] = NAN;   // a NaN among the corners of the mixed cells round a voxel that lay just outside the surface

    int64_t nq = -1;
    const int64_t nv = fluid_sdf_mesh(&g, 0, 0, nullptr, nullptr, &nq);
    REQUIRE(nv > 100 && nq > 100);
    REQUIRE(fluid_sdf_mesh_normals(&g, 0, nullptr) == nv);
    std::vector<float> nr((size_t)3 * nv, 7.0f);
    REQUIRE(fluid_sdf_mesh_normals(&g, nv - 1, nr.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_sdf_mesh_normals(nullptr, nv, nr.data()) == -FLUID_ERR_ARG);
    for (float c : nr) REQUIRE(c == 7.0f);   // nothing written
    REQUIRE(fluid_sdf_mesh_normals(&g, nv, nr.data()) == nv);
    int64_t unit = 0, zero = 0;
    for (int64_t i = 0; i < nv; ++i) {
        const double l2 = (double)nr[3 * i] * nr[3 * i] + (double)nr[3 * i + 1] * nr[3 * i + 1] + (double)nr[3 * i + 2] * nr[3 * i + 2];
        REQUIRE(std::isfinite(l2));
        if (l2 == 0.0) ++zero;
        else {
            REQUIRE(std::fabs(l2 - 1.0) <= 1e-6);
            ++unit;
        }
    }
    REQUIRE(unit > 100 && zero >= 1);   // the NaN's cells give +0 normals

    std::vector<float> vert((size_t)3 * nv);
    std::vector<uint32_t> quad((size_t)4 * nq);
    REQUIRE(fluid_sdf_mesh(&g, nv, nq, vert.data(), quad.data(), nullptr) == nv);
    const fluid_mesh_t m{n, nv, nq, 3.0f, 1.0f, bg, vert.data(), quad.data()};
    REQUIRE(fluid_mesh_triangles(&m, 0, nullptr) == 2 * nq);
    std::vector<uint32_t> tri((size_t)6 * nq, 9u);
    REQUIRE(fluid_mesh_triangles(&m, 2 * nq - 1, tri.data()) == -FLUID_ERR_ARG);
    REQUIRE(fluid_mesh_triangles(nullptr, 2 * nq, tri.data()) == -FLUID_ERR_ARG);
    const uint32_t keep = quad[5];
    quad[5] = (uint32_t)nv;
    REQUIRE(fluid_mesh_triangles(&m, 2 * nq, tri.data()) == -FLUID_ERR_ARG);
    quad[5] = keep;
    for (uint32_t c : tri) REQUIRE(c == 9u);   // nothing written
    REQUIRE(fluid_mesh_triangles(&m, 2 * nq, tri.data()) == 2 * nq);
    for (uint32_t c : tri) REQUIRE((int64_t)c < nv);
    const fluid_mesh_t empty{n, 0, 0, 3.0f, 1.0f, bg, nullptr, nullptr};
    REQUIRE(fluid_mesh_triangles(&empty, 0, nullptr) == 0 && fluid_mesh_triangles(&empty, 0, tri.data()) == 0);

    std::vector<float> vel((size_t)3 * nv, 0.5f);
    for (unsigned what = 0; what < 8; ++what) {
        const fluid_mesh_ex_t ex{(what & FLUID_MESH_VELOCITY) ? vel.data() : nullptr, (what & FLUID_MESH_NORMALS) ? nr.data() : nullptr,
                                 (what & FLUID_MESH_TRIANGLES) ? tri.data() : nullptr, (what & FLUID_MESH_TRIANGLES) ? 2 * nq : 0};
        const std::string path = dir + "/san_normals" + std::to_string(what) + ".ply";
        REQUIRE(fluid_write_ply_mesh_ex(path.c_str(), &m, &ex, 0.5f, 2.0f) == FLUID_OK);
        const long rec = 12 * (1 + (what & 1) + ((what >> 1) & 1)), faces = (what & 4) ? 26 * nq : 17 * nq;
        const long size = file_size(path);
        REQUIRE(size > rec * nv + faces && size < rec * nv + faces + 500);
    }
    REQUIRE(fluid_write_ply_mesh_ex((dir + "/san_normals_null.ply").c_str(), &m, nullptr, 0.5f, 2.0f) == FLUID_OK);
    REQUIRE(file_size(dir + "/san_normals_null.ply") == file_size(dir + "/san_normals0.ply"));
    const std::string bad = dir + "/san_normals_bad.ply";
    const fluid_mesh_ex_t odd{nullptr, nullptr, tri.data(), 2 * nq - 1}, nan_scale{vel.data(), nullptr, nullptr, 0};
    REQUIRE(fluid_write_ply_mesh_ex(bad.c_str(), &m, &odd, 0.5f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_ex(bad.c_str(), &m, &nan_scale, 0.5f, NAN) == FLUID_ERR_ARG);
    tri[4] = (uint32_t)nv;
    const fluid_mesh_ex_t beyond{nullptr, nr.data(), tri.data(), 2 * nq};
    REQUIRE(fluid_write_ply_mesh_ex(bad.c_str(), &m, &beyond, 0.5f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(fluid_write_ply_mesh_ex(bad.c_str(), &m, &beyond, 0.0f, 1.0f) == FLUID_ERR_ARG);
    REQUIRE(file_size(bad) < 0);
    const fluid_mesh_ex_t normals_only{nullptr, nr.data(), nullptr, 0};
    REQUIRE(fluid_write_ply_mesh_ex((dir + "/no_such_dir/m.ply").c_str(), &m, &normals_only, 0.5f, 1.0f) == FLUID_ERR_ARG);
    const fluid_mesh_ex_t empty_parts{nullptr, nr.data(), tri.data(), 0};   // an empty mesh: the pointers only select the header lines
    REQUIRE(fluid_write_ply_mesh_ex((dir + "/san_normals_empty.ply").c_str(), &empty, &empty_parts, 1.0f, 1.0f) == FLUID_OK);

    std::swap(origin[0], origin[3]);   // (no longer ascending)
    std::swap(origin[1], origin[4]);
    std::swap(origin[2], origin[5]);
    REQUIRE(fluid_sdf_mesh_normals(&g, 0, nullptr) == -FLUID_ERR_ARG);
    printf("host sanitizer run (normals): ok %lld %lld\n", (long long)nv, (long long)nq);
    return 0;
}
