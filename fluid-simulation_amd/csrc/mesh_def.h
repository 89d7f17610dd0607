// The per-cell arithmetic of the surface nets (include/fluid_hip.h, "liquid surface as a mesh", "liquid surface, attributes",
// "normals and triangles"), stated once for the kernels (kernels_mesh.hip, hipcc) and the host functions (mesh_host.cpp, g++): a
// cell's inside mask and owned edges, each of its 12 edges, the vertex, its velocity and normal, an owned edge's quad, a quad's
// two triangles.  A cell is a pointer to its min corner in a 9^3 tile, [(lx * 9 + ly) * 9 + lz]; how the tile is filled, how a vertex
// is numbered and where things are written is each side's own.  Both builds state -ffp-contract=off; every product is formed before
// its sum.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define MDEF __host__ __device__ __forceinline__
#else
#define MDEF inline
#endif

namespace mdef {

constexpr int TILE = 9 * 9 * 9;

struct Vec3 {
    float x, y, z;
};

// The cell with min corner (px, py, pz) and the three edges that leave that corner towards +x, +y, +z; g: whatever holds the
// grid's lo and hi.  Returns the inside mask of the 8 corners (bit dx*4 + dy*2 + dz); mixed = the cell exists and its corners
// disagree; edges bit a = the owned edge along axis a gives a quad (its ends disagree and the four cells round it exist).  A cell
// that owns such an edge is mixed.
template <typename Grid>
MDEF unsigned cell(const Grid& g, const float* c, int px, int py, int pz, bool& mixed, unsigned& edges)
{
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) m |= (c[(d >> 2) * 81 + ((d >> 1) & 1) * 9 + (d & 1)] < 0.0f ? 1u : 0u) << d;
    const bool cx = px >= g.lo && px <= g.hi - 1, cy = py >= g.lo && py <= g.hi - 1, cz = pz >= g.lo && pz <= g.hi - 1;        // the cell's axis range
    const bool qx = px >= g.lo + 1 && cx, qy = py >= g.lo + 1 && cy, qz = pz >= g.lo + 1 && cz;                                // ... and the cell at -1 too
    mixed = cx && cy && cz && m != 0 && m != 255;
    const unsigned in0 = m & 1;
    edges = 0;
    if (cx && qy && qz && ((m >> 4) & 1) != in0) edges |= 1;
    if (cy && qz && qx && ((m >> 2) & 1) != in0) edges |= 2;
    if (cz && qx && qy && ((m >> 1) & 1) != in0) edges |= 4;
    return m;
}

// One counting edge's share of the vertex velocity: A[axis * TILE + i] the staged velocities, B[i] the active bits, i0, i1 the
// ends' places in the tile.  An edge with no active end has no share.
MDEF void edge_velocity(const float* A, const unsigned char* B, int i0, int i1, float t, float* s, int& kv)
{
    const bool b0 = B[i0] != 0, b1 = B[i1] != 0;
    if (!b0 && !b1) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float a0 = A[a * TILE + i0], a1 = A[a * TILE + i1];
        float e;
        if (b0 && b1) {
            const float d = a1 - a0;
            const float td = t * d;
            e = a0 + td;
        } else e = b0 ? a0 : a1;
        s[a] += e;
    }
    ++kv;
}

// Edge e = 0..11 of the definition's order: axis a = e / 4 (x, y, z), then the two other axes, ascending, at (0,0), (0,1), (1,0),
// (1,1).  If its ends disagree in sign it counts: k grows, its crossing t = v0 / (v0 - v1) adds to the offset sums sx, sy, sz, and
// with VEL its share (edge_velocity; c0 = the min corner's place in the tile) to sv and kv.  All sums start from zero, and the walk is
// `for (e = 0; e < 12; ++e)` at the caller: only one edge's body is stated here, and values go in and out as plain arguments, because
// the compiler finishes an inlined function before it inlines it, and a loop unrolled in here reaches the kernel with the operands of
// its sums in another order than the kernel's own loop gives (profiles/mesh/NOTES.md).
template <bool VEL>
MDEF void edge(const float* c, int e, const float* A, const unsigned char* B, int c0, float& sx, float& sy, float& sz, float* sv, int& k, int& kv)
{
    const int stride[3] = {81, 9, 1};
    const int a = e >> 2, d1 = (e >> 1) & 1, d2 = e & 1;
    const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
    const int i0 = d1 * stride[b1] + d2 * stride[b2], i1 = i0 + stride[a];
    const float v0 = c[i0], v1 = c[i1];
    if ((v0 < 0.0f) != (v1 < 0.0f)) {
        const float t = v0 / (v0 - v1);
        sx += a == 0 ? t : (float)d1, sy += a == 1 ? t : (float)(a == 0 ? d1 : d2), sz += a == 2 ? t : (float)d2, ++k;
        if (VEL) edge_velocity(A, B, c0 + i0, c0 + i1, t, sv, kv);
    }
}

// the vertex's offset f[3] in its cell and its position from the walk's sums; kf = (float)k, the edges that counted
MDEF void vertex(float sx, float sy, float sz, float kf, int px, int py, int pz, float* f, float* out)
{
    f[0] = sx / kf;
    out[0] = (float)px + f[0];
    f[1] = sy / kf;
    out[1] = (float)py + f[1];
    f[2] = sz / kf;
    out[2] = (float)pz + f[2];
}

// the vertex velocity from the shares' sums: +0 where no edge had one
MDEF void velocity(const float* s, int kv, float* out)
{
    const float kvf = (float)kv;
    out[0] = kv ? s[0] / kvf : 0.0f;
    out[1] = kv ? s[1] / kvf : 0.0f;
    out[2] = kv ? s[2] / kvf : 0.0f;
}

// Term o = 0..3 of the gradient of the trilinear interpolant of the cell's eight corners at the offset f[3]: per axis the edge at
// (0,0), (0,1), (1,0), (1,1) of the two other axes, ascending, weighted by those axes' offsets.  The sum is `for (o = 0; o < 4; ++o)`
// from zero at the caller, as for edge.
MDEF Vec3 gradient_term(const float* c, const float* f, int o, Vec3 g)
{
    const float fx = f[0], fy = f[1], fz = f[2];
    const float ex = 1.0f - fx, ey = 1.0f - fy, ez = 1.0f - fz;
    const int d1 = o >> 1, d2 = o & 1;
    const float wx = (d1 ? fy : ey) * (d2 ? fz : ez);
    const float wy = (d1 ? fx : ex) * (d2 ? fz : ez);
    const float wz = (d1 ? fx : ex) * (d2 ? fy : ey);
    const float dx = c[81 + d1 * 9 + d2] - c[d1 * 9 + d2];
    const float dy = c[d1 * 81 + 9 + d2] - c[d1 * 81 + d2];
    const float dz = c[d1 * 81 + d2 * 9 + 1] - c[d1 * 81 + d2 * 9];
    g.x = g.x + wx * dx;
    g.y = g.y + wy * dy;
    g.z = g.z + wz * dz;
    return g;
}

// the unit normal from the gradient: +0 where its length is 0 or NaN
MDEF Vec3 unit(Vec3 g)
{
    float l2 = g.x * g.x;
    l2 = l2 + g.y * g.y;
    l2 = l2 + g.z * g.z;
    const float len = sqrtf(l2);
    const bool some = len > 0.0f;   // (false for a NaN too)
    Vec3 n;
    n.x = some ? g.x / len : 0.0f;
    n.y = some ? g.y / len : 0.0f;
    n.z = some ? g.z / len : 0.0f;
    return n;
}

// The quad of the owned edge along axis a of the cell p: with (b, c) = the two other axes in cyclic order its four cells are
// Q0 = p - e_b - e_c, Q1 = p - e_c, Q2 = p, Q3 = p - e_b.  Q[0], Q[1], Q[3] = the min corners of the three others.
MDEF void quad_cells(int a, int px, int py, int pz, int (*Q)[3])
{
    const int bx = a == 2, by = a == 0, bz = a == 1;
    const int cx = a == 1, cy = a == 2, cz = a == 0;
    Q[0][0] = px - bx - cx, Q[0][1] = py - by - cy, Q[0][2] = pz - bz - cz;
    Q[1][0] = px - cx, Q[1][1] = py - cy, Q[1][2] = pz - cz;
    Q[3][0] = px - bx, Q[3][1] = py - by, Q[3][2] = pz - bz;
}
// ... and the order of the four vertex numbers: by the sign of the edge's min corner (bit 0 of the inside mask)
MDEF void quad_order(unsigned m, unsigned q0, unsigned q1, unsigned q2, unsigned q3, unsigned* q)
{
    const bool inside = m & 1;
    q[0] = q0, q[1] = inside ? q1 : q3, q[2] = q2, q[3] = inside ? q3 : q1;
}

MDEF float dist2(const float* p0, const float* p1)
{
    const float x = p1[0] - p0[0], y = p1[1] - p0[1], z = p1[2] - p0[2];
    float s = x * x;
    s = s + y * y;
    s = s + z * z;
    return s;
}
// Quad (a, b, c, d) with the vertex positions p0..p3 -> two triangles at t[0..5], cut along the shorter diagonal: d13 < d02 gives
// (a, b, d), (b, c, d); otherwise, ties and NaN included, (a, b, c), (a, c, d).
MDEF void quad_triangles(const unsigned* q, const float* p0, const float* p1, const float* p2, const float* p3, unsigned* t)
{
    const float d02 = dist2(p0, p2), d13 = dist2(p1, p3);
    const bool cut13 = d13 < d02;
    t[0] = q[0], t[1] = q[1], t[2] = cut13 ? q[3] : q[2];
    t[3] = cut13 ? q[1] : q[0], t[4] = q[2], t[5] = q[3];
}

}  // namespace mdef
