// The liquid surface as a mesh on the host (include/fluid_hip.h, "liquid surface as a mesh", "liquid surface, attributes", "normals
// and triangles") — no GPU, no HIP, no OpenVDB.  The per-cell arithmetic is mesh_def.h's, the same text the kernels
// (kernels_mesh.hip) compile; the list's rules, the leaves worked on and the tile loader are leaf_list.h's; the PLY body and the
// triangles are ply_mesh.h's.  This file is the host's way to fetch and to place: one walk over a leaf list, every unlisted leaf
// being +bg.  A mixed cell has an inside corner, which lies in a listed leaf; its min corner lies in that leaf or in one of the seven
// leaves at -1: those are the leaves worked on, in ascending order, each with its 9^3 values (the +1 faces from up to seven
// neighbours, found by bisection in the sorted list).  The place of a vertex or a quad is a running count, because the order of the
// definition is the order of the walk.  No dense grid.
//   fluid_sdf_mesh          vertices and quads: how a decomposed run gets its mesh (after fluid_sdf_grids_merge).  Two walks: masks
//                           and counts, then the arrays.
//   fluid_sdf_mesh_attr     the vertex velocities of fluid_sdf_mesh(grid) in its vertex order; the only way a hand-made list can
//                           drive the arithmetic into the rule for an edge with no active end.
//   fluid_sdf_mesh_normals  the vertex normals; the only way a hand-made list can drive it into a NaN or a zero gradient.
//   fluid_sdf_attr_to_dense ids and velocities of a leaf list on the dense grid.
//   fluid_mesh_triangles, fluid_write_ply_mesh, fluid_write_ply_mesh_attr, fluid_write_ply_mesh_ex   check their arguments here.
// Arithmetic: float, no contraction (the build states -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "leaf_list.h"
#include "mesh_def.h"
#include "ply_mesh.h"

namespace {

using mdef::TILE;

// the 9^3 tile of a worked-on leaf: [(lx * 9 + ly) * 9 + lz] = the voxel o + (lx, ly, lz), 0 <= lx, ly, lz <= 8
struct Tile {
    int lo, hi;            // the grid
    float V[TILE];         // values, +bg where no leaf is listed
    float A[3 * TILE];     // where asked for: velocities, [axis * TILE + place]
    uint8_t B[TILE];       //                  active bits
};

// at: nullptr, or the attributes to stage beside the values
void load(Tile& t, const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, const Org& o)
{
    std::fill(t.V, t.V + TILE, g->background);
    if (at) std::fill(t.A, t.A + 3 * TILE, 0.0f), std::fill(t.B, t.B + TILE, (uint8_t)0);
    load_tile(g, o, [&](long l, int off, int i) {
        t.V[i] = g->values[512 * (size_t)l + off];
        if (!at) return;
        t.B[i] = (uint8_t)((g->active[8 * (size_t)l + (off >> 6)] >> (off & 63)) & 1u);
        for (int a = 0; a < 3; ++a) t.A[a * TILE + i] = at->velocity[1536 * (size_t)l + 512 * a + off];
    });
}

// one mixed cell of the walk
struct Cell {
    const Tile& t;
    size_t leaf;          // its leaf's index in the work list
    int off;              // its min corner's offset in that leaf
    int i;                //                   place in the tile
    const float* c;       // = t.V + i
    int px, py, pz;       // its min corner
    unsigned m, edges;    // mdef::cell
    int64_t number;       // of its vertex: the mixed cells before it
};

// f(Cell) for every mixed cell of the (checked) list in the definition's order; returns how many there are
template <typename F>
int64_t walk(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, const std::vector<Org>& work, F f)
{
    std::vector<Tile> holder(1);   // (12 KB, the velocities and bits staged or not: not on the stack of whoever calls)
    Tile& t = holder[0];
    t.lo = -(g->n / 2), t.hi = t.lo + g->n - 1;
    int64_t nv = 0;
    for (size_t w = 0; w < work.size(); ++w) {
        load(t, g, at, work[w]);
        for (int off = 0; off < 512; ++off) {
            const int x = off >> 6, y = (off >> 3) & 7, z = off & 7;
            const int i = (x * 9 + y) * 9 + z;
            const int px = work[w].x + x, py = work[w].y + y, pz = work[w].z + z;
            bool mixed;
            unsigned edges;
            const unsigned m = mdef::cell(t, t.V + i, px, py, pz, mixed, edges);
            if (!mixed) continue;   // (and owns no edge)
            f(Cell{t, w, off, i, t.V + i, px, py, pz, m, edges, nv});
            ++nv;
        }
    }
    return nv;
}

// The walk over a cell's 12 edges (mesh_def.h states one edge; the loop is the caller's): the offset f[3] of its vertex and, where
// asked for, its position, and its velocity from the staged velocities and active bits.
void vertex_of(const Cell& c, float* f, float* position, float* velocity)
{
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv[3] = {0.0f, 0.0f, 0.0f}, p[3];
    int k = 0, kv = 0;
    for (int e = 0; e < 12; ++e) {
        if (velocity) mdef::edge<true>(c.c, e, c.t.A, c.t.B, c.i, sx, sy, sz, sv, k, kv);
        else mdef::edge<false>(c.c, e, nullptr, nullptr, c.i, sx, sy, sz, sv, k, kv);
    }
    mdef::vertex(sx, sy, sz, (float)k, c.px, c.py, c.pz, f, position ? position : p);
    if (velocity) mdef::velocity(sv, kv, velocity);
}

// The shape of fluid_sdf_mesh_attr and fluid_sdf_mesh_normals: one walk counts (nothing is written before the cap is known to
// hold), a second calls emit(cell, out + 3 * its vertex number).
template <typename Emit>
int64_t per_vertex(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, int64_t cap_vertices, float* out, Emit emit)
{
    const std::vector<Org> work = mesh_work_list(g);
    const int64_t nv = walk(g, nullptr, work, [](const Cell&) {});
    if (nv > 0x7fffffffLL) return -FLUID_ERR_ARG;
    if (!out) return nv;
    if (nv > cap_vertices) return -FLUID_ERR_ARG;
    walk(g, at, work, [&](const Cell& c) { emit(c, out + 3 * (size_t)c.number); });
    return nv;
}

int check_attr(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* a)
{
    if (check_list(g) != FLUID_OK || !a || a->n_leaves != g->n_leaves) return FLUID_ERR_ARG;
    if (g->n_leaves > 0 && (!a->id || !a->velocity)) return FLUID_ERR_ARG;
    return FLUID_OK;
}

int check_mesh(const char* path, const fluid_mesh_t* m, float voxel_size)
{
    if (!path || !m || m->n_vertices < 0 || m->n_quads < 0 || !(voxel_size > 0.0f)) return FLUID_ERR_ARG;
    if ((m->n_vertices > 0 && !m->vertices) || (m->n_quads > 0 && !m->quads)) return FLUID_ERR_ARG;
    return FLUID_OK;
}

}  // namespace

extern "C" {

int64_t fluid_sdf_mesh(const fluid_sdf_grid_t* g, int64_t cap_vertices, int64_t cap_quads, float* vertices, uint32_t* quads, int64_t* n_quads)
{
    if (check_list(g) != FLUID_OK || (vertices == nullptr) != (quads == nullptr)) return -FLUID_ERR_ARG;
    const std::vector<Org> work = mesh_work_list(g);
    struct Leaf {
        uint64_t mask[8];   // the mixed cells of the leaf
        int64_t vbase;      // number of its first vertex
    };
    std::vector<Leaf> leaf(work.size());
    int64_t nq = 0;
    const int64_t nv = walk(g, nullptr, work, [&](const Cell& c) {
        leaf[c.leaf].mask[c.off >> 6] |= 1ull << (c.off & 63);
        nq += __builtin_popcount(c.edges);
    });
    if (nv > 0x7fffffffLL || nq > 0x7fffffffLL) return -FLUID_ERR_ARG;
    if (vertices) {
        if (nv > cap_vertices || nq > cap_quads) return -FLUID_ERR_ARG;
        int64_t base = 0;
        for (Leaf& l : leaf) {
            l.vbase = base;
            for (uint64_t w : l.mask) base += __builtin_popcountll(w);
        }
        // number of the vertex of the (mixed) cell with min corner p
        const auto number = [&](const int* p) -> uint32_t {
            const Org o{floor_to(p[0], LEAF), floor_to(p[1], LEAF), floor_to(p[2], LEAF)};
            const auto it = std::lower_bound(work.begin(), work.end(), o);
            if (it == work.end() || !(*it == o)) return 0xffffffffu;   // (cannot be: a mixed cell's leaf is worked on)
            const Leaf& l = leaf[it - work.begin()];
            const int off = ((p[0] & 7) * 8 + (p[1] & 7)) * 8 + (p[2] & 7);
            int64_t r = l.vbase;
            for (int w = 0; w < (off >> 6); ++w) r += __builtin_popcountll(l.mask[w]);
            r += __builtin_popcountll(l.mask[off >> 6] & ((1ull << (off & 63)) - 1ull));
            return (uint32_t)r;
        };
        uint32_t* q = quads;
        walk(g, nullptr, work, [&](const Cell& c) {
            float f[3];
            vertex_of(c, f, vertices + 3 * (size_t)c.number, nullptr);
            for (int a = 0; a < 3; ++a) {
                if (!((c.edges >> a) & 1)) continue;
                int Q[4][3];
                mdef::quad_cells(a, c.px, c.py, c.pz, Q);
                mdef::quad_order(c.m, number(Q[0]), number(Q[1]), (uint32_t)c.number, number(Q[3]), q);
                q += 4;
            }
        });
    }
    if (n_quads) *n_quads = nq;
    return nv;
}

int64_t fluid_sdf_mesh_attr(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, int64_t cap_vertices, float* velocity)
{
    if (check_attr(g, at) != FLUID_OK) return -FLUID_ERR_ARG;
    return per_vertex(g, at, cap_vertices, velocity, [](const Cell& c, float* out) {
        float f[3];
        vertex_of(c, f, nullptr, out);
    });
}

int64_t fluid_sdf_mesh_normals(const fluid_sdf_grid_t* g, int64_t cap_vertices, float* normals)
{
    if (check_list(g) != FLUID_OK) return -FLUID_ERR_ARG;
    return per_vertex(g, nullptr, cap_vertices, normals, [](const Cell& c, float* out) {
        float f[3];
        vertex_of(c, f, nullptr, nullptr);
        mdef::Vec3 g3 = {0.0f, 0.0f, 0.0f};
        for (int o = 0; o < 4; ++o) g3 = mdef::gradient_term(c.c, f, o, g3);
        const mdef::Vec3 n = mdef::unit(g3);
        out[0] = n.x, out[1] = n.y, out[2] = n.z;
    });
}

int64_t fluid_mesh_triangles(const fluid_mesh_t* m, int64_t cap_triangles, uint32_t* triangles) { return mesh_triangles(m, cap_triangles, triangles); }

int fluid_sdf_attr_to_dense(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* at, uint32_t* id, float* velocity)
{
    if (check_attr(g, at) != FLUID_OK) return FLUID_ERR_ARG;
    const size_t n3 = (size_t)g->n * g->n * g->n;
    if (id) std::fill(id, id + n3, (uint32_t)FLUID_SDF_NO_ID);
    if (velocity) std::fill(velocity, velocity + 3 * n3, 0.0f);
    scatter_leaves(g, [&](size_t l, int off, size_t c) {
        if (id) id[c] = at->id[512 * l + off];
        if (velocity)
            for (int a = 0; a < 3; ++a) velocity[a * n3 + c] = at->velocity[1536 * l + 512 * a + off];
    });
    return FLUID_OK;
}

int fluid_write_ply_mesh(const char* path, const fluid_mesh_t* m, float voxel_size)
{
    if (check_mesh(path, m, voxel_size) != FLUID_OK) return FLUID_ERR_ARG;
    return write_ply(path, m, voxel_size, false, nullptr, 0.0f);
}

int fluid_write_ply_mesh_attr(const char* path, const fluid_mesh_t* m, const fluid_mesh_attr_t* at, float voxel_size, float velocity_scale)
{
    if (!at || check_mesh(path, m, voxel_size) != FLUID_OK || !std::isfinite(velocity_scale)) return FLUID_ERR_ARG;
    if (at->n_vertices != m->n_vertices) return FLUID_ERR_ARG;
    if (m->n_vertices > 0 && !at->velocity) return FLUID_ERR_ARG;
    return write_ply(path, m, voxel_size, true, at->velocity, velocity_scale);
}

int fluid_write_ply_mesh_ex(const char* path, const fluid_mesh_t* m, const fluid_mesh_ex_t* ex, float voxel_size, float velocity_scale)
{
    if (check_mesh(path, m, voxel_size) != FLUID_OK) return FLUID_ERR_ARG;
    const float* vel = ex ? ex->velocity : nullptr;
    const float* nrm = ex ? ex->normals : nullptr;
    const uint32_t* tri = ex ? ex->triangles : nullptr;
    if (vel && !std::isfinite(velocity_scale)) return FLUID_ERR_ARG;
    if (tri && ex->n_triangles != 2 * m->n_quads) return FLUID_ERR_ARG;
    return write_ply(path, m, voxel_size, vel != nullptr, vel, velocity_scale, nrm, tri);
}

}  // extern "C"
