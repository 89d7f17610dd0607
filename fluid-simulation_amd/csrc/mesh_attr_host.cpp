// The liquid surface's attributes on the host (include/fluid_hip.h, "liquid surface, attributes") — no GPU, no HIP, no OpenVDB.
// It walks as mesh_host.cpp does: the leaves worked on and the tile loader are leaf_list.h's, the PLY body is ply_mesh.h's.
//   fluid_sdf_mesh_attr        the vertex velocities of fluid_sdf_mesh(grid) in its vertex order: the same leaves are worked on
//                              (the listed ones and their neighbours at -1), in the same ascending order, each with its 9^3 values,
//                              active bits and velocities (the +1 faces from up to seven neighbours, found by bisection).  One
//                              pass: the order of the definition is the order of the walk.  No dense grid.  This is the second
//                              implementation the kernel (kernels_mesh.hip, k_mesh_emit<true>) is compared with, and the only one
//                              a hand-made list can drive into the rule for an edge with no active end.
//   fluid_sdf_attr_to_dense    ids and velocities of a leaf list on the dense grid.
//   fluid_write_ply_mesh_attr  binary little-endian PLY with vx / vy / vz per vertex.
//   fluid_sdf_mesh_normals     ("normals and triangles") the vertex normals of fluid_sdf_mesh(grid): the same walk with the values
//                              alone in the tile.  The second implementation k_mesh_emit<., true> is compared with, and the only
//                              one a hand-made list can drive into a NaN or a zero gradient.
//   fluid_mesh_triangles, fluid_write_ply_mesh_ex   their bodies are ply_mesh.h's.
// Arithmetic: float, no contraction (the build states -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "leaf_list.h"
#include "ply_mesh.h"

namespace {

constexpr int TILE = 9 * 9 * 9;

int check_attr(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* a)
{
    if (check_list(g) != FLUID_OK || !a || a->n_leaves != g->n_leaves) return FLUID_ERR_ARG;
    if (g->n_leaves > 0 && (!a->id || !a->velocity)) return FLUID_ERR_ARG;
    return FLUID_OK;
}

struct Tile {
    const fluid_sdf_grid_t* g;
    const fluid_sdf_attr_t* at;
    int lo, hi;
    float V[TILE];        // values, +bg where no leaf is listed
    float A[3][TILE];     // velocities
    uint8_t B[TILE];      // active bits

    // [(lx * 9 + ly) * 9 + lz] = the voxel o + (lx, ly, lz), 0 <= lx, ly, lz <= 8
    void load(const Org& o)
    {
        for (int i = 0; i < TILE; ++i) V[i] = g->background, A[0][i] = A[1][i] = A[2][i] = 0.0f, B[i] = 0;
        load_tile(g, o, [&](long l, int off, int i) {
            V[i] = g->values[512 * (size_t)l + off];
            B[i] = (uint8_t)((g->active[8 * (size_t)l + (off >> 6)] >> (off & 63)) & 1u);
            for (int a = 0; a < 3; ++a) A[a][i] = at->velocity[1536 * (size_t)l + 512 * a + off];
        });
    }
    bool mixed(int i, int px, int py, int pz) const
    {
        unsigned m = 0;
        for (int d = 0; d < 8; ++d) m |= (V[i + (d >> 2) * 81 + ((d >> 1) & 1) * 9 + (d & 1)] < 0.0f ? 1u : 0u) << d;
        const bool cx = px >= lo && px <= hi - 1, cy = py >= lo && py <= hi - 1, cz = pz >= lo && pz <= hi - 1;
        return cx && cy && cz && m != 0 && m != 255;
    }
    // the velocity of the vertex of the (mixed) cell whose min corner is place i of the tile
    void vertex(int i, float* out) const
    {
        float s[3] = {0.0f, 0.0f, 0.0f};
        int kv = 0;
        static const int stride[3] = {81, 9, 1};
        for (int a = 0; a < 3; ++a) {
            const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;   // the two other axes, ascending
            for (int o = 0; o < 4; ++o) {
                const int d1 = o >> 1, d2 = o & 1;
                const int i0 = i + d1 * stride[b1] + d2 * stride[b2], i1 = i0 + stride[a];
                const float v0 = V[i0], v1 = V[i1];
                if ((v0 < 0.0f) == (v1 < 0.0f)) continue;
                const bool a0 = B[i0] != 0, a1 = B[i1] != 0;
                if (!a0 && !a1) continue;
                const float den = v0 - v1;
                const float t = v0 / den;
                for (int c = 0; c < 3; ++c) {
                    float e;
                    if (a0 && a1) {
                        const float d = A[c][i1] - A[c][i0];
                        const float td = t * d;
                        e = A[c][i0] + td;
                    } else e = a0 ? A[c][i0] : A[c][i1];
                    s[c] += e;
                }
                ++kv;
            }
        }
        const float kf = (float)kv;
        for (int c = 0; c < 3; ++c) out[c] = kv ? s[c] / kf : 0.0f;
    }
};

// the walk of fluid_sdf_mesh_attr with the values alone: what fluid_sdf_mesh_normals needs
struct NormalTile {
    const fluid_sdf_grid_t* g;
    int lo, hi;
    float V[TILE];

    void load(const Org& o)
    {
        for (int i = 0; i < TILE; ++i) V[i] = g->background;
        load_tile(g, o, [&](long l, int off, int i) { V[i] = g->values[512 * (size_t)l + off]; });
    }
    bool mixed(int i, int px, int py, int pz) const
    {
        unsigned m = 0;
        for (int d = 0; d < 8; ++d) m |= (V[i + (d >> 2) * 81 + ((d >> 1) & 1) * 9 + (d & 1)] < 0.0f ? 1u : 0u) << d;
        const bool cx = px >= lo && px <= hi - 1, cy = py >= lo && py <= hi - 1, cz = pz >= lo && pz <= hi - 1;
        return cx && cy && cz && m != 0 && m != 255;
    }
    // the normal of the vertex of the (mixed) cell whose min corner is place i of the tile
    void normal(int i, float* out) const
    {
        static const int stride[3] = {81, 9, 1};
        // the vertex's offset in its cell, as mesh_host.cpp forms it
        float s[3] = {0.0f, 0.0f, 0.0f};
        int k = 0;
        for (int a = 0; a < 3; ++a) {
            const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
            for (int o = 0; o < 4; ++o) {
                const int d1 = o >> 1, d2 = o & 1;
                const int i0 = i + d1 * stride[b1] + d2 * stride[b2];
                const float v0 = V[i0], v1 = V[i0 + stride[a]];
                if ((v0 < 0.0f) == (v1 < 0.0f)) continue;
                const float den = v0 - v1;
                const float t = v0 / den;
                s[a] += t;
                s[b1] += (float)d1;
                s[b2] += (float)d2;
                ++k;
            }
        }
        const float kf = (float)k;
        const float f[3] = {s[0] / kf, s[1] / kf, s[2] / kf};
        const float e[3] = {1.0f - f[0], 1.0f - f[1], 1.0f - f[2]};
        float g3[3];
        for (int a = 0; a < 3; ++a) {
            const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
            float ga = 0.0f;
            for (int o = 0; o < 4; ++o) {
                const int d1 = o >> 1, d2 = o & 1;
                const int i0 = i + d1 * stride[b1] + d2 * stride[b2];
                const float w1 = d1 ? f[b1] : e[b1], w2 = d2 ? f[b2] : e[b2];
                const float w = w1 * w2;
                const float dv = V[i0 + stride[a]] - V[i0];
                const float wd = w * dv;
                ga = ga + wd;
            }
            g3[a] = ga;
        }
        float l2 = g3[0] * g3[0];
        const float yy = g3[1] * g3[1], zz = g3[2] * g3[2];
        l2 = l2 + yy;
        l2 = l2 + zz;
        const float len = std::sqrt(l2);
        const bool some = len > 0.0f;   // (false for a NaN too)
        for (int a = 0; a < 3; ++a) out[a] = some ? g3[a] / len : 0.0f;
    }
};

}  // namespace

extern "C" {

int64_t fluid_sdf_mesh_normals(const fluid_sdf_grid_t* g, int64_t cap_vertices, float* normals)
{
    if (check_list(g) != FLUID_OK) return -FLUID_ERR_ARG;
    NormalTile me;
    me.g = g;
    me.lo = -(g->n / 2), me.hi = me.lo + g->n - 1;
    const std::vector<Org> work = mesh_work_list(g);
    // pass 0 counts (nothing is written before the cap is known to hold), pass 1 writes
    int64_t nv = 0;
    for (int pass = 0; pass < (normals ? 2 : 1); ++pass) {
        if (pass == 1 && nv > cap_vertices) return -FLUID_ERR_ARG;
        int64_t k = 0;
        for (const Org& w : work) {
            me.load(w);
            for (int off = 0; off < 512; ++off) {
                const int x = off >> 6, y = (off >> 3) & 7, z = off & 7;
                const int i = (x * 9 + y) * 9 + z;
                if (!me.mixed(i, w.x + x, w.y + y, w.z + z)) continue;
                if (pass == 1) me.normal(i, normals + 3 * (size_t)k);
                ++k;
            }
        }
        nv = k;
        if (nv > 0x7fffffffLL) return -FLUID_ERR_ARG;
    }
    return nv;
}

int64_t fluid_mesh_triangles(const fluid_mesh_t* m, int64_t cap_triangles, uint32_t* triangles) { return mesh_triangles(m, cap_triangles, triangles); }

int fluid_write_ply_mesh_ex(const char* path, const fluid_mesh_t* m, const fluid_mesh_ex_t* ex, float voxel_size, float velocity_scale)
{
    if (!path || !m || m->n_vertices < 0 || m->n_quads < 0 || !(voxel_size > 0.0f)) return FLUID_ERR_ARG;
    if ((m->n_vertices > 0 && !m->vertices) || (m->n_quads > 0 && !m->quads)) return FLUID_ERR_ARG;
    const float* vel = ex ? ex->velocity : nullptr;
    const float* nrm = ex ? ex->normals : nullptr;
    const uint32_t* tri = ex ? ex->triangles : nullptr;
    if (vel && !std::isfinite(velocity_scale)) return FLUID_ERR_ARG;
    if (tri && ex->n_triangles != 2 * m->n_quads) return FLUID_ERR_ARG;
    return write_ply(path, m, voxel_size, vel != nullptr, vel, velocity_scale, nrm, tri);
}

int64_t fluid_sdf_mesh_attr(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, int64_t cap_vertices, float* velocity)
{
    if (check_attr(g, at) != FLUID_OK) return -FLUID_ERR_ARG;
    std::vector<Tile> holder(1);   // (13 KB: not on the stack of whoever calls)
    Tile& me = holder[0];
    me.g = g, me.at = at;
    me.lo = -(g->n / 2), me.hi = me.lo + g->n - 1;
    const std::vector<Org> work = mesh_work_list(g);
    // pass 0 counts (nothing is written before the cap is known to hold), pass 1 writes
    int64_t nv = 0;
    for (int pass = 0; pass < (velocity ? 2 : 1); ++pass) {
        if (pass == 1 && nv > cap_vertices) return -FLUID_ERR_ARG;
        int64_t k = 0;
        for (const Org& w : work) {
            me.load(w);
            for (int off = 0; off < 512; ++off) {
                const int x = off >> 6, y = (off >> 3) & 7, z = off & 7;
                const int i = (x * 9 + y) * 9 + z;
                if (!me.mixed(i, w.x + x, w.y + y, w.z + z)) continue;
                if (pass == 1) me.vertex(i, velocity + 3 * (size_t)k);
                ++k;
            }
        }
        nv = k;
        if (nv > 0x7fffffffLL) return -FLUID_ERR_ARG;
    }
    return nv;
}

int fluid_sdf_attr_to_dense(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, uint32_t* id, float* velocity)
{
    if (check_attr(g, at) != FLUID_OK) return FLUID_ERR_ARG;
    const int n = g->n, lo = -(n / 2), hi = lo + n - 1;
    const size_t n3 = (size_t)n * n * n;
    if (id) std::fill(id, id + n3, (uint32_t)FLUID_SDF_NO_ID);
    if (velocity) std::fill(velocity, velocity + 3 * n3, 0.0f);
    for (int l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        for (int off = 0; off < 512; ++off) {
            const int x = o[0] + (off >> 6), y = o[1] + ((off >> 3) & 7), z = o[2] + (off & 7);
            if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) continue;
            const size_t c = ((size_t)(x - lo) * n + (size_t)(y - lo)) * n + (size_t)(z - lo);
            if (id) id[c] = at->id[512 * (size_t)l + off];
            if (velocity)
                for (int a = 0; a < 3; ++a) velocity[a * n3 + c] = at->velocity[1536 * (size_t)l + 512 * a + off];
        }
    }
    return FLUID_OK;
}

int fluid_write_ply_mesh_attr(const char* path, const fluid_mesh_t* m, const fluid_mesh_attr_t* at, float voxel_size, float velocity_scale)
{
    if (!path || !m || !at || m->n_vertices < 0 || m->n_quads < 0 || !(voxel_size > 0.0f) || !std::isfinite(velocity_scale)) return FLUID_ERR_ARG;
    if (at->n_vertices != m->n_vertices) return FLUID_ERR_ARG;
    if ((m->n_vertices > 0 && (!m->vertices || !at->velocity)) || (m->n_quads > 0 && !m->quads)) return FLUID_ERR_ARG;
    return write_ply(path, m, voxel_size, true, at->velocity, velocity_scale);
}

}  // extern "C"
