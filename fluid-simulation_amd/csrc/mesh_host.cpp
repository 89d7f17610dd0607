// The liquid surface as a mesh on the host (include/fluid_hip.h, "liquid surface as a mesh") — no GPU, no HIP, no OpenVDB.  The
// list's rules, the leaves worked on and the tile loader are leaf_list.h's, the PLY body is ply_mesh.h's.
//   fluid_sdf_mesh        surface nets of a leaf list, every unlisted leaf being +bg: how a decomposed run gets its mesh (after
//                         fluid_sdf_grids_merge), and the second implementation the kernels (kernels_mesh.hip) are compared with.
//                         A mixed cell has an inside corner, which lies in a listed leaf; its min corner lies in that leaf or in
//                         one of the seven leaves at -1: those are the leaves worked on, in ascending order, each with its 9^3
//                         values (the +1 faces from up to seven neighbours, found by bisection in the sorted list).  Two passes:
//                         masks and counts, then vertices and quads; the place of either is a running count, because the order of
//                         the definition is the order of the walk.  No dense grid.
//   fluid_write_ply_mesh  binary little-endian PLY.
// Arithmetic: float, no contraction (x86-64 has none without -mfma; the sanitizer build states -ffp-contract=off).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "leaf_list.h"
#include "ply_mesh.h"

namespace {

struct Work {
    Org o;
    uint64_t mask[8];   // the mixed cells of the leaf
    int64_t vbase;      // number of its first vertex
};

struct Mesher {
    const fluid_sdf_grid_t* g;
    int lo, hi;
    std::vector<Work> work;
    float V[9 * 9 * 9];

    // V[(lx * 9 + ly) * 9 + lz] = val(o + (lx, ly, lz)), 0 <= lx, ly, lz <= 8
    void load(const Org& o)
    {
        for (float& v : V) v = g->background;
        load_tile(g, o, [&](long l, int off, int i) { V[i] = g->values[512 * (size_t)l + off]; });
    }
    // the cell with min corner p and the edges p owns: the corners' inside mask (bit dx*4 + dy*2 + dz)
    unsigned cell(const float* c, int px, int py, int pz, bool& mixed, unsigned& edges) const
    {
        unsigned m = 0;
        for (int d = 0; d < 8; ++d) m |= (c[(d >> 2) * 81 + ((d >> 1) & 1) * 9 + (d & 1)] < 0.0f ? 1u : 0u) << d;
        const bool cx = px >= lo && px <= hi - 1, cy = py >= lo && py <= hi - 1, cz = pz >= lo && pz <= hi - 1;
        const bool qx = px >= lo + 1 && cx, qy = py >= lo + 1 && cy, qz = pz >= lo + 1 && cz;
        mixed = cx && cy && cz && m != 0 && m != 255;
        const unsigned in0 = m & 1;
        edges = 0;
        if (cx && qy && qz && ((m >> 4) & 1) != in0) edges |= 1;
        if (cy && qz && qx && ((m >> 2) & 1) != in0) edges |= 2;
        if (cz && qx && qy && ((m >> 1) & 1) != in0) edges |= 4;
        return m;
    }
    static void vertex(const float* c, int px, int py, int pz, float* out)
    {
        float s[3] = {0.0f, 0.0f, 0.0f};
        int k = 0;
        static const int stride[3] = {81, 9, 1};
        for (int a = 0; a < 3; ++a) {
            const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;   // the two other axes, ascending
            for (int o = 0; o < 4; ++o) {
                const int d1 = o >> 1, d2 = o & 1;
                const float v0 = c[d1 * stride[b1] + d2 * stride[b2]], v1 = c[d1 * stride[b1] + d2 * stride[b2] + stride[a]];
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
        const float q[3] = {s[0] / kf, s[1] / kf, s[2] / kf};
        out[0] = (float)px + q[0];
        out[1] = (float)py + q[1];
        out[2] = (float)pz + q[2];
    }
    // number of the vertex of the (mixed) cell with min corner (cx, cy, cz)
    uint32_t number(int cx, int cy, int cz) const
    {
        const Org o{floor_to(cx, LEAF), floor_to(cy, LEAF), floor_to(cz, LEAF)};
        const auto it = std::lower_bound(work.begin(), work.end(), o, [](const Work& w, const Org& k) { return w.o < k; });
        if (it == work.end() || !(it->o == o)) return 0xffffffffu;   // (cannot be: a mixed cell's leaf is worked on)
        const int off = ((cx & 7) * 8 + (cy & 7)) * 8 + (cz & 7);
        int64_t r = it->vbase;
        for (int w = 0; w < (off >> 6); ++w) r += __builtin_popcountll(it->mask[w]);
        r += __builtin_popcountll(it->mask[off >> 6] & ((1ull << (off & 63)) - 1ull));
        return (uint32_t)r;
    }
    // pass 0 (vertices == NULL): masks, bases, counts.  pass 1: the arrays.
    void pass(float* vertices, uint32_t* quads, int64_t& nv, int64_t& nq)
    {
        nv = nq = 0;
        for (Work& w : work) {
            load(w.o);
            if (!vertices) {
                memset(w.mask, 0, sizeof w.mask);
                w.vbase = nv;
            }
            for (int off = 0; off < 512; ++off) {
                const int x = off >> 6, y = (off >> 3) & 7, z = off & 7;
                const int px = w.o.x + x, py = w.o.y + y, pz = w.o.z + z;
                const float* c = V + (x * 9 + y) * 9 + z;
                bool mixed;
                unsigned edges;
                const unsigned m = cell(c, px, py, pz, mixed, edges);
                if (mixed) {
                    if (vertices) vertex(c, px, py, pz, vertices + 3 * (size_t)nv);
                    else w.mask[off >> 6] |= 1ull << (off & 63);
                    ++nv;
                }
                for (int a = 0; a < 3; ++a) {
                    if (!((edges >> a) & 1)) continue;
                    if (quads) {
                        int eb[3] = {0, 0, 0}, ec[3] = {0, 0, 0};
                        eb[(a + 1) % 3] = 1;
                        ec[(a + 2) % 3] = 1;
                        const uint32_t q0 = number(px - eb[0] - ec[0], py - eb[1] - ec[1], pz - eb[2] - ec[2]);
                        const uint32_t q1 = number(px - ec[0], py - ec[1], pz - ec[2]);
                        const uint32_t q2 = number(px, py, pz);
                        const uint32_t q3 = number(px - eb[0], py - eb[1], pz - eb[2]);
                        uint32_t* q = quads + 4 * (size_t)nq;
                        q[0] = q0, q[2] = q2;
                        q[1] = (m & 1) ? q1 : q3;
                        q[3] = (m & 1) ? q3 : q1;
                    }
                    ++nq;
                }
            }
        }
    }
};

}  // namespace

extern "C" {

int64_t fluid_sdf_mesh(const fluid_sdf_grid_t* g, int64_t cap_vertices, int64_t cap_quads, float* vertices, uint32_t* quads, int64_t* n_quads)
{
    if (check_list(g) != FLUID_OK || (vertices == nullptr) != (quads == nullptr)) return -FLUID_ERR_ARG;
    Mesher me;
    me.g = g;
    me.lo = -(g->n / 2), me.hi = me.lo + g->n - 1;
    for (const Org& o : mesh_work_list(g)) me.work.push_back(Work{o, {}, 0});
    int64_t nv = 0, nq = 0;
    me.pass(nullptr, nullptr, nv, nq);
    if (nv > 0x7fffffffLL || nq > 0x7fffffffLL) return -FLUID_ERR_ARG;
    if (vertices) {
        if (nv > cap_vertices || nq > cap_quads) return -FLUID_ERR_ARG;
        int64_t v2 = 0, q2 = 0;
        me.pass(vertices, quads, v2, q2);
    }
    if (n_quads) *n_quads = nq;
    return nv;
}

int fluid_write_ply_mesh(const char* path, const fluid_mesh_t* m, float voxel_size)
{
    if (!path || !m || m->n_vertices < 0 || m->n_quads < 0 || !(voxel_size > 0.0f)) return FLUID_ERR_ARG;
    if ((m->n_vertices > 0 && !m->vertices) || (m->n_quads > 0 && !m->quads)) return FLUID_ERR_ARG;
    return write_ply(path, m, voxel_size, false, nullptr, 0.0f);
}

}  // extern "C"
