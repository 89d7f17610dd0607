// Surface nets of the particles' level set for gfx950 (wave64): one vertex per grid cell whose eight corners disagree in sign, one
// quad per grid edge whose two ends disagree in sign, no case table (include/fluid_hip.h, "liquid surface as a mesh";
// fluid_mesh.hip).  The kernels work on what k_sdf_search (kernels_sdf.hip) leaves on the device: tv (512 values) and a listed
// flag per leaf j = (jx * nl[1] + jy) * nl[2] + jz of the range, the particles' base-cell box dilated by 4 cells and clipped to the
// grid.  A leaf whose flag is 0 is +bg everywhere WHATEVER its tv holds (the search leaves early and writes the flag alone, so the
// values may be those of an earlier snapshot), and so is every leaf outside the range: only flagged leaves' tv is ever read.
//
// Every leaf of the range is processed, not only the listed ones, and no leaf outside it needs to be.  A voxel is inside (< 0)
// only if it is less than R <= 3 from a counted particle (w >= 1 and R + w <= 4), so within 3 cells (Chebyshev) of that particle's
// base cell (|p - round(p)| <= 0.5).  A mixed cell has an inside corner, and its min corner is that corner minus {0,1}^3: within
// [-4, +3] cells of the base cell.  The range holds the base cells' box dilated by 4, clipped to the grid, and a cell exists only
// inside the grid: every mixed cell's min corner lies in a leaf of the range.  The same holds for the four cells round an edge
// with a sign change (each has that edge's inside end as a corner), so a quad's vertex numbers are looked up inside the range.
//
//   mark   one 512-thread block per leaf of the range, thread t = the voxel ((x&7)*8 + (y&7))*8 + (z&7) = the cell with that min
//          corner = the owner of the three edges that leave the voxel towards +x, +y, +z.  The leaf's 9^3 values go to LDS, the
//          +1 faces from up to seven neighbour leaves (index arithmetic on j).  Out: the mixed-cell mask (8 words by ballot,
//          wave = x plane), the exclusive prefix of the words' popcounts, the vertex and the quad count of the leaf.  A leaf
//          with no listed leaf among itself and the seven leaves at +1 has neither and leaves at once.
//   totals one block sums the leaves' counts in 64 bits and writes min(sum, 2^31) for either: what the host reads back to size the
//          slot, and to refuse a mesh whose 32-bit bases would wrap.  (A first form added the counts to two words by
//          compare-and-swap from k_mesh_mark: the blocks queued on them, 1.9 ms at 256^3 against 14 us for k_mesh_emit.)
//   (two exclusive scans of the counts on the host side give the leaves' bases)
//   emit   same tiling.  A mixed cell's vertex goes to vbase[leaf] + its rank in the mask; a quad to qbase[leaf] + the quads of
//          lower voxels (ballots of the three edge bits) — position alone decides the place, there is no ordering by arrival.  The
//          number of a vertex in a neighbour leaf at -1 is vbase[leaf'] + the popcount of that leaf's stored mask below the cell.
//   emit<true> ("liquid surface, attributes") also writes a velocity per vertex from the search's per-voxel velocities and masks.
//   emit<., true> ("normals and triangles") also writes a unit normal per vertex: the gradient of the trilinear interpolant of the
//          cell's eight corners at the vertex's offset in its cell, from the tile the block has staged anyway.
//   tris   a launch of its own behind emit (a quad's vertices may be another block's of the same emit launch): one thread per
//          quad, its 16 bytes and its four vertices in, two triangles cut along the shorter diagonal out.
// What happens in a cell — mask and owned edges, each of the 12 edges, vertex, velocity, normal, quad, triangles — is mesh_def.h's, the
// text mesh_host.cpp compiles too; these kernels are how the device fetches a tile (LDS), numbers a vertex (ballots, cmask / cpre /
// vbase) and writes.  Arithmetic of a vertex: include/fluid_hip.h; float, no FMA (-ffp-contract=off), the division correctly rounded
// (-fhip-fp32-correctly-rounded-divide-sqrt).
#include "common.h"
#include "mesh_def.h"

namespace fl {

constexpr int MESH_V = mdef::TILE;

struct MeshLeaf {
    long j;
    int jx, jy, jz;   // leaf of the range
    int ox, oy, oz;   // its origin
};

__device__ __forceinline__ MeshLeaf mesh_leaf(const SdfGeom& g)
{
    MeshLeaf l;
    l.j = blockIdx.x;
    l.jz = (int)(l.j % g.nl[2]), l.jy = (int)((l.j / g.nl[2]) % g.nl[1]), l.jx = (int)(l.j / ((long)g.nl[1] * g.nl[2]));
    l.ox = g.L0 + 8 * (g.l0[0] + l.jx), l.oy = g.L0 + 8 * (g.l0[1] + l.jy), l.oz = g.L0 + 8 * (g.l0[2] + l.jz);
    return l;
}

// index of the leaf (jx, jy, jz) of the range, or -1: outside the range
__device__ __forceinline__ long mesh_range_index(const SdfGeom& g, int jx, int jy, int jz)
{
    if (jx < 0 || jx >= g.nl[0] || jy < 0 || jy >= g.nl[1] || jz < 0 || jz >= g.nl[2]) return -1;
    return ((long)jx * g.nl[1] + jy) * g.nl[2] + jz;
}

// V[(lx * 9 + ly) * 9 + lz] = val(origin + (lx, ly, lz)), lx, ly, lz in 0..8: +bg wherever the leaf is unlisted or outside the range
__device__ __forceinline__ void mesh_load(const SdfGeom& g, const MeshLeaf& l, const float* __restrict__ tv, const int* __restrict__ flags,
                                          float* V)
{
    for (int i = threadIdx.x; i < MESH_V; i += 512) {
        const int lz = i % 9, ly = (i / 9) % 9, lx = i / 81;
        const long q = mesh_range_index(g, l.jx + (lx >> 3), l.jy + (ly >> 3), l.jz + (lz >> 3));
        float v = g.bg;
        if (q >= 0 && flags[q]) v = tv[q * 512 + (((lx & 7) * 8 + (ly & 7)) * 8 + (lz & 7))];
        V[i] = v;
    }
}

__global__ __launch_bounds__(512) void k_mesh_mark(SdfGeom g, const float* __restrict__ tv, const int* __restrict__ flags,
                                                   unsigned long long* __restrict__ cmask, int* __restrict__ cpre, int* __restrict__ vcnt,
                                                   int* __restrict__ qcnt)
{
    __shared__ float V[MESH_V];
    __shared__ int wv[8], wq[8];
    const int t = threadIdx.x;
    const MeshLeaf l = mesh_leaf(g);
    bool listed = false;
    if (t < 8) {
        const long q = mesh_range_index(g, l.jx + (t >> 2), l.jy + ((t >> 1) & 1), l.jz + (t & 1));
        listed = q >= 0 && flags[q] != 0;
    }
    if (!__syncthreads_or(listed)) {   // +bg in all 9^3: no mixed cell, no edge with a sign change
        if (t < 8) cmask[l.j * 8 + t] = 0, cpre[l.j * 8 + t] = 0;
        if (t == 0) vcnt[l.j] = 0, qcnt[l.j] = 0;
        return;
    }
    mesh_load(g, l, tv, flags, V);
    __syncthreads();
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    bool mixed;
    unsigned edges;
    mdef::cell(g, V + (x * 9 + y) * 9 + z, l.ox + x, l.oy + y, l.oz + z, mixed, edges);
    const unsigned long long b = __ballot(mixed);
    const int nq = __popcll(__ballot(edges & 1)) + __popcll(__ballot(edges & 2)) + __popcll(__ballot(edges & 4));
    if ((t & 63) == 0) {
        cmask[l.j * 8 + x] = b;
        wv[x] = __popcll(b);
        wq[x] = nq;
    }
    __syncthreads();
    if (t < 8) {
        int pre = 0;
        for (int k = 0; k < t; ++k) pre += wv[k];
        cpre[l.j * 8 + t] = pre;
    }
    if (t == 0) {
        int nv = 0, nqs = 0;
        for (int k = 0; k < 8; ++k) nv += wv[k], nqs += wq[k];
        vcnt[l.j] = nv;
        qcnt[l.j] = nqs;
    }
}

// tot[0] = min(sum of vcnt, 2^31), tot[1] = the same of qcnt; one block, sums in 64 bits (a leaf gives at most 512 and 1536)
__global__ __launch_bounds__(1024) void k_mesh_totals(long n, const int* __restrict__ vcnt, const int* __restrict__ qcnt, unsigned* __restrict__ tot)
{
    __shared__ unsigned long long sv[16], sq[16];
    unsigned long long v = 0, q = 0;
    for (long i = threadIdx.x; i < n; i += 1024) v += (unsigned)vcnt[i], q += (unsigned)qcnt[i];
    v = wave_sum(v);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v, sq[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = q = 0;
        for (int k = 0; k < 16; ++k) v += sv[k], q += sq[k];
        tot[0] = v > 0x80000000ull ? 0x80000000u : (unsigned)v;
        tot[1] = q > 0x80000000ull ? 0x80000000u : (unsigned)q;
    }
}

// number of the vertex of the (mixed) cell with min corner (cx, cy, cz); 0xffffffff if its leaf lay outside the range (header: it cannot)
__device__ __forceinline__ unsigned mesh_vertex_number(const SdfGeom& g, int cx, int cy, int cz, const unsigned long long* __restrict__ cmask,
                                                       const int* __restrict__ cpre, const int* __restrict__ vbase)
{
    const long q = mesh_range_index(g, ((cx - g.L0) >> 3) - g.l0[0], ((cy - g.L0) >> 3) - g.l0[1], ((cz - g.L0) >> 3) - g.l0[2]);
    if (q < 0) return 0xffffffffu;
    const int off = ((cx & 7) * 8 + (cy & 7)) * 8 + (cz & 7);
    const unsigned long long below = cmask[q * 8 + (off >> 6)] & ((1ull << (off & 63)) - 1ull);
    return (unsigned)(vbase[q] + cpre[q * 8 + (off >> 6)] + __popcll(below));
}

// ATTR: beside the values the block stages the velocities (3 x 9^3 floats) and the active bits (one byte each) of the same up to
// eight leaves, not active wherever the leaf is unflagged or outside the range (the search's tm / tvel of such a leaf are stale or
// do not exist); each mixed cell's thread writes its vertex velocity to the place its vertex goes.
// NORMALS: each mixed cell's thread also writes the unit normal of its vertex (include/fluid_hip.h, "normals and triangles") from
// the offsets it has just formed and the eight corners in V: no further LDS, loads or atomics.
template <bool ATTR, bool NORMALS>
__global__ __launch_bounds__(512) void k_mesh_emit(SdfGeom g, const float* __restrict__ tv, const int* __restrict__ flags,
                                                   const unsigned long long* __restrict__ cmask, const int* __restrict__ cpre,
                                                   const int* __restrict__ vcnt, const int* __restrict__ qcnt, const int* __restrict__ vbase,
                                                   const int* __restrict__ qbase, float* __restrict__ vertices, uint4* __restrict__ quads,
                                                   const unsigned long long* __restrict__ tm, const float* __restrict__ tvel,
                                                   float* __restrict__ vvel, float* __restrict__ vnrm)
{
    __shared__ float V[MESH_V];
    __shared__ float A[ATTR ? 3 * MESH_V : 1];
    __shared__ unsigned char B[ATTR ? MESH_V : 1];
    __shared__ int wq[8];
    const int t = threadIdx.x;
    const MeshLeaf l = mesh_leaf(g);
    if (vcnt[l.j] == 0 && qcnt[l.j] == 0) return;   // (the whole block alike)
    mesh_load(g, l, tv, flags, V);
    if (ATTR) {
        for (int i = t; i < MESH_V; i += 512) {
            const int lz = i % 9, ly = (i / 9) % 9, lx = i / 81;
            const long q = mesh_range_index(g, l.jx + (lx >> 3), l.jy + (ly >> 3), l.jz + (lz >> 3));
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            unsigned char b = 0;
            if (q >= 0 && flags[q]) {
                const int off = ((lx & 7) * 8 + (ly & 7)) * 8 + (lz & 7);
                b = (unsigned char)((tm[q * 8 + (off >> 6)] >> (off & 63)) & 1ull);
                const float* tw = tvel + q * 1536 + off;
                a0 = tw[0], a1 = tw[512], a2 = tw[1024];
            }
            A[i] = a0, A[MESH_V + i] = a1, A[2 * MESH_V + i] = a2;
            B[i] = b;
        }
    }
    __syncthreads();
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const int px = l.ox + x, py = l.oy + y, pz = l.oz + z;
    const float* c = V + (x * 9 + y) * 9 + z;
    bool mixed;
    unsigned edges;
    const unsigned m = mdef::cell(g, c, px, py, pz, mixed, edges);
    const unsigned long long lt = (1ull << (t & 63)) - 1ull;
    const unsigned long long b = __ballot(mixed), bx = __ballot(edges & 1), by = __ballot(edges & 2), bz = __ballot(edges & 4);
    if ((t & 63) == 0) wq[x] = __popcll(bx) + __popcll(by) + __popcll(bz);
    __syncthreads();
    if (mixed) {
        int kv = 0, k = 0;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv[3] = {0.0f, 0.0f, 0.0f};
        const int c0 = (x * 9 + y) * 9 + z;   // the cell's min corner in the tile
#pragma unroll
        for (int e = 0; e < 12; ++e) mdef::edge<ATTR>(c, e, A, B, c0, sx, sy, sz, sv, k, kv);
        const float kf = (float)k;
        const size_t vn = (size_t)(vbase[l.j] + cpre[l.j * 8 + x] + __popcll(b & lt));
        float f[3];   // the vertex's offset in its cell
        mdef::vertex(sx, sy, sz, kf, px, py, pz, f, vertices + 3 * vn);
        if (NORMALS) {
            mdef::Vec3 g = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int o = 0; o < 4; ++o) g = mdef::gradient_term(c, f, o, g);
            const mdef::Vec3 n = mdef::unit(g);
            float* on = vnrm + 3 * vn;
            on[0] = n.x, on[1] = n.y, on[2] = n.z;
        }
        if (ATTR) mdef::velocity(sv, kv, vvel + 3 * vn);
    }
    if (edges) {
        size_t at = (size_t)qbase[l.j] + __popcll(bx & lt) + __popcll(by & lt) + __popcll(bz & lt);
        for (int k = 0; k < x; ++k) at += wq[k];
        const unsigned q2 = mesh_vertex_number(g, px, py, pz, cmask, cpre, vbase);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((edges >> a) & 1)) continue;
            int Q[4][3];
            mdef::quad_cells(a, px, py, pz, Q);
            const unsigned q0 = mesh_vertex_number(g, Q[0][0], Q[0][1], Q[0][2], cmask, cpre, vbase);
            const unsigned q1 = mesh_vertex_number(g, Q[1][0], Q[1][1], Q[1][2], cmask, cpre, vbase);
            const unsigned q3 = mesh_vertex_number(g, Q[3][0], Q[3][1], Q[3][2], cmask, cpre, vbase);
            unsigned q[4];
            mdef::quad_order(m, q0, q1, q2, q3, q);
            quads[at++] = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
}

// Triangles ("normals and triangles"): thread i owns quad i = (a, b, c, d) and writes triangles 2i and 2i + 1, cut along the shorter
// diagonal of the vertex positions (d13 < d02: (a, b, d), (b, c, d); otherwise, ties and NaN included: (a, b, c), (a, c, d)).  tris
// is 16-byte aligned (fluid_mesh.hip puts it right behind the quads), so quad i's 24-byte record starts at a multiple of 8 for every
// i and at a multiple of 16 for even i: one 16-byte and one 8-byte store, in the order the record's alignment allows.  An entry
// >= nv cannot come from emit (mesh_vertex_number's header); the guard keeps a wrong number from reading out of the slot.
__global__ __launch_bounds__(256) void k_mesh_tris(long nq, long nv, const uint4* __restrict__ quads, const float* __restrict__ vertices,
                                                   uint2* __restrict__ tris)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const uint4 q = quads[i];
    const unsigned e[4] = {q.x, q.y, q.z, q.w};
    float P[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t at = (long)e[k] < nv ? 3 * (size_t)e[k] : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) P[k][a] = vertices[at + a];
    }
    unsigned t[6];
    mdef::quad_triangles(e, P[0], P[1], P[2], P[3], t);
    uint2* out = tris + 3 * i;
    if (i & 1) {
        out[0] = make_uint2(t[0], t[1]);
        *(uint4*)(out + 1) = make_uint4(t[2], t[3], t[4], t[5]);
    } else {
        *(uint4*)out = make_uint4(t[0], t[1], t[2], t[3]);
        out[2] = make_uint2(t[4], t[5]);
    }
}

void launch_mesh_mark(hipStream_t st, const SdfGeom& g, const float* tv, const int* flags, uint64_t* cmask, int* cpre, int* vcnt, int* qcnt,
                      unsigned* tot)
{
    hipLaunchKernelGGL(k_mesh_mark, dim3((unsigned)g.leaves()), dim3(512), 0, st, g, tv, flags, (unsigned long long*)cmask, cpre, vcnt, qcnt);
    hipLaunchKernelGGL(k_mesh_totals, dim3(1), dim3(1024), 0, st, g.leaves(), (const int*)vcnt, (const int*)qcnt, tot);
}

// tm / tvel / vvel: non-NULL for a velocity per vertex; vnrm: non-NULL for a normal per vertex
void launch_mesh_emit(hipStream_t st, const SdfGeom& g, const float* tv, const int* flags, const uint64_t* tm, const float* tvel,
                      const uint64_t* cmask, const int* cpre, const int* vcnt, const int* qcnt, const int* vbase, const int* qbase, float* vertices,
                      uint32_t* quads, float* vvel, float* vnrm)
{
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)g.leaves()), dim3(512), 0, st, g, tv, flags, (const unsigned long long*)cmask, cpre, vcnt, qcnt, vbase,
                           qbase, vertices, (uint4*)quads, (const unsigned long long*)tm, tvel, vvel, vnrm);
    };
    if (vvel) vnrm ? go(k_mesh_emit<true, true>) : go(k_mesh_emit<true, false>);
    else vnrm ? go(k_mesh_emit<false, true>) : go(k_mesh_emit<false, false>);
}

void launch_mesh_tris(hipStream_t st, long nq, long nv, const uint32_t* quads, const float* vertices, uint32_t* tris)
{
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_mesh_tris, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, nq, nv, (const uint4*)quads, vertices, (uint2*)tris);
}

}  // namespace fl
