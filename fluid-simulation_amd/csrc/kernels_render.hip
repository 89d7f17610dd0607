// Ray caster for the particles' level set, gfx950 (wave64): include/fluid_hip.h, "liquid surface as an image"; fluid_render.hip.  The
// kernels work on what the front half of a surface snapshot leaves on the device: tv (512 values) and a listed flag per leaf
// j = (jx * nl[1] + jy) * nl[2] + jz of the range.  A leaf whose flag is 0 is +bg everywhere WHATEVER its tv holds, and so is every
// leaf outside the range (kernels_mesh.hip's header: every voxel < 0 lies in the range): only flagged leaves' tv is ever read.
//
//   neg    one wave per leaf of the range: neg[j] = the leaf is flagged and holds a value < 0 (8 values per lane, one ballot).
//   occ    the cell with min corner c reads corners from the leaves L(c) + {0,1}^3, and c runs from lo - 1, one leaf below the range
//          when lo is a multiple of 8: occ lives on the range extended by one leaf towards -x, -y, -z, RenderGeom::ne leaves per
//          axis, as a bit list (one thread per 32-bit word): occ(L) = OR of neg over L + {0,1}^3, 0 where that leaves the range.
//   march  one wave per 8 x 8 pixel tile, four tiles (16 x 16 pixels) per block.  A lane walks its ray's samples k = 0, 1, ...; the
//          definition's p_k is formed for every k the lane looks at, by render_def.h's functions, the ones the host uses.
//
// Which samples may be left out.  A sample counts only if value(p_k) < 0, which needs a corner < 0, which needs p_k inside the box E =
// (the cells of the extended range) n (the definition's bounds [lo - 1, hi + 1)) AND occ of its cell's leaf set.  Every sample that
// is left out is shown to be outside E or in a leaf with occ == 0 by forming a p_k' EXACTLY and using that each p_k,a is monotone in
// k (k -> (float)k * step -> t_near + . -> . * d_a -> eye_a + . are all monotone roundings; k <= 65536 is exact in float):
//   - p_k in a leaf box B with occ == 0: a float estimate proposes k' > k near the ray's exit from B; if p_k' lies in B, so do all
//     samples between (per axis between two values of one interval), and the walk resumes at k' + 1.  If not: k + 1.
//   - p_k outside E on an axis it moves away on (or not at all): every later sample is outside too; the pixel is a miss.
//   - p_k outside E otherwise: an estimate proposes k' near the entry; if p_k' is still outside E on an axis a with the ray moving
//     towards E on a, so are all samples before it; resume at k' + 1.  If not: k + 1.
// The estimates use float division and may be anything — NaN and infinity included, they are clamped as floats before the
// conversion —: only the exact test of p_k' decides, so over-conservative means slower, never different.  At a hit v0 =
// value(p_{k-1}) is evaluated by the formula wherever p_{k-1} lies.
// The occ bits are read through the caches (4 KB at 256^3); LDS staging of bits or values waits for a measurement.
// Arithmetic: float, no FMA (-ffp-contract=off), division and sqrtf correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).
#include "common.h"
#include "render_def.h"

namespace fl {

__global__ __launch_bounds__(256) void k_render_neg(long leaves, const float* __restrict__ tv, const int* __restrict__ flags,
                                                    unsigned char* __restrict__ neg)
{
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= leaves) return;   // (a whole wave alike)
    const int lane = threadIdx.x & 63;
    bool any = false;
    if (flags[j]) {
        const float4* v = (const float4*)(tv + j * 512) + lane * 2;
        const float4 a = v[0], b = v[1];
        any = a.x < 0.0f || a.y < 0.0f || a.z < 0.0f || a.w < 0.0f || b.x < 0.0f || b.y < 0.0f || b.z < 0.0f || b.w < 0.0f;
    }
    const unsigned long long m = __ballot(any);
    if (lane == 0) neg[j] = m != 0ull;
}

__global__ __launch_bounds__(256) void k_render_occ(RenderGeom r, const unsigned char* __restrict__ neg, unsigned* __restrict__ occ)
{
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = r.ext_leaves();
    if (w * 32 >= total) return;
    unsigned bits = 0;
    for (int b = 0; b < 32; ++b) {
        const long e = w * 32 + b;
        if (e >= total) break;
        const int ez = (int)(e % r.ne[2]), ey = (int)((e / r.ne[2]) % r.ne[1]), ex = (int)(e / ((long)r.ne[1] * r.ne[2]));
        bool any = false;
        for (int d = 0; d < 8; ++d) {
            const int jx = ex - 1 + (d >> 2), jy = ey - 1 + ((d >> 1) & 1), jz = ez - 1 + (d & 1);   // leaf of the range
            if (jx < 0 || jx >= r.g.nl[0] || jy < 0 || jy >= r.g.nl[1] || jz < 0 || jz >= r.g.nl[2]) continue;
            any = any || neg[((long)jx * r.g.nl[1] + jy) * r.g.nl[2] + jz] != 0;
        }
        bits |= (any ? 1u : 0u) << b;
    }
    occ[w] = bits;
}

// val(c): +bg outside the grid, outside the range and in an unflagged leaf
__device__ __forceinline__ float render_val(const SdfGeom& g, const float* __restrict__ tv, const int* __restrict__ flags, int x, int y, int z)
{
    if (x < g.lo || x > g.hi || y < g.lo || y > g.hi || z < g.lo || z > g.hi) return g.bg;
    const int jx = ((x - g.L0) >> 3) - g.l0[0], jy = ((y - g.L0) >> 3) - g.l0[1], jz = ((z - g.L0) >> 3) - g.l0[2];
    if (jx < 0 || jx >= g.nl[0] || jy < 0 || jy >= g.nl[1] || jz < 0 || jz >= g.nl[2]) return g.bg;
    const long q = ((long)jx * g.nl[1] + jy) * g.nl[2] + jz;
    if (!flags[q]) return g.bg;
    return tv[q * 512 + (((x & 7) * 8 + (y & 7)) * 8 + (z & 7))];
}

__device__ __forceinline__ void render_corners(const SdfGeom& g, const float* __restrict__ tv, const int* __restrict__ flags, const int* c, float* v)
{
#pragma unroll
    for (int d = 0; d < 8; ++d) v[d] = render_val(g, tv, flags, c[0] + (d >> 2), c[1] + ((d >> 1) & 1), c[2] + (d & 1));
}

// value(p) of the definition, wherever p lies
__device__ __forceinline__ float render_value(const SdfGeom& g, const float* __restrict__ tv, const int* __restrict__ flags, const float* p)
{
    if (!rdef::in_bounds(p, g.lo, g.hi)) return g.bg;
    int c[3];
    float f[3], v[8];
    rdef::cell_of(p, c, f);
    render_corners(g, tv, flags, c, v);
    return rdef::trilinear(v, f);
}

// a float estimate as a sample index in (k, n_steps - 1], or k: no proposal.  Any input, NaN and infinity included
__device__ __forceinline__ int render_propose(const fluid_camera_t& c, float t_est, int k)
{
    float kf = floorf((t_est - c.t_near) / c.step) - 1.0f;
    if (!(kf > (float)k)) return k;
    kf = fminf(kf, (float)(c.n_steps - 1));
    return (int)kf;
}

__global__ __launch_bounds__(256) void k_render_march(RenderGeom r, fluid_camera_t cam, fluid_shade_t sh, const float* __restrict__ tv,
                                                      const int* __restrict__ flags, const unsigned* __restrict__ occ, unsigned* __restrict__ hits,
                                                      unsigned char* __restrict__ rgb, float* __restrict__ depth, float* __restrict__ normals)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool mine = i < cam.width && j < cam.height;
    const SdfGeom& g = r.g;
    float d[3] = {0.0f, 0.0f, 0.0f}, t = INFINITY, n[3] = {0.0f, 0.0f, 0.0f};
    bool hit = false;
    if (mine && r.any && rdef::ray_dir(cam, i, j, d)) {
        const float E0[3] = {(float)r.e0[0], (float)r.e0[1], (float)r.e0[2]}, E1[3] = {(float)r.e1[0], (float)r.e1[1], (float)r.e1[2]};
        int k = 0;
        while (k < cam.n_steps) {
            const float tk = rdef::sample_t(cam, k);
            float p[3];
            rdef::point_at(cam, d, tk, p);
            const bool in_e = p[0] >= E0[0] && p[0] < E1[0] && p[1] >= E0[1] && p[1] < E1[1] && p[2] >= E0[2] && p[2] < E1[2];
            if (!in_e) {
                // outside for good?  (a NaN component is neither: the walk goes on sample by sample)
                bool gone = false;
                float t_in = 0.0f;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    gone = gone || (p[a] >= E1[a] && d[a] >= 0.0f) || (p[a] < E0[a] && d[a] <= 0.0f);
                    if (p[a] < E0[a] && d[a] > 0.0f) t_in = fmaxf(t_in, (E0[a] - cam.eye[a]) / d[a]);
                    if (p[a] >= E1[a] && d[a] < 0.0f) t_in = fmaxf(t_in, (E1[a] - cam.eye[a]) / d[a]);
                }
                if (gone) break;
                int kn = k + 1;
                const int kp = render_propose(cam, t_in, k);
                if (kp > k) {
                    float q[3];
                    rdef::point_at(cam, d, rdef::sample_t(cam, kp), q);
                    bool before = false;   // q is outside E on an axis the ray still moves towards E on: so is every sample up to kp
#pragma unroll
                    for (int a = 0; a < 3; ++a) before = before || (q[a] < E0[a] && d[a] > 0.0f) || (q[a] >= E1[a] && d[a] < 0.0f);
                    if (before) kn = kp + 1;
                }
                k = kn;
                continue;
            }
            int c[3];
            float f[3];
            rdef::cell_of(p, c, f);
            // the cell's leaf in the extended range: in_e puts every index in [0, ne)
            const int ex = ((c[0] - g.L0) >> 3) - g.l0[0] + 1, ey = ((c[1] - g.L0) >> 3) - g.l0[1] + 1, ez = ((c[2] - g.L0) >> 3) - g.l0[2] + 1;
            const long e = ((long)ex * r.ne[1] + ey) * r.ne[2] + ez;
            if (!((occ[e >> 5] >> (e & 31)) & 1u)) {
                // the leaf's box, clipped to E
                const int o[3] = {g.L0 + 8 * (g.l0[0] + ex - 1), g.L0 + 8 * (g.l0[1] + ey - 1), g.L0 + 8 * (g.l0[2] + ez - 1)};
                float B0[3], B1[3], t_out = INFINITY;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    B0[a] = fmaxf((float)o[a], E0[a]), B1[a] = fminf((float)(o[a] + 8), E1[a]);
                    if (d[a] > 0.0f) t_out = fminf(t_out, (B1[a] - cam.eye[a]) / d[a]);
                    if (d[a] < 0.0f) t_out = fminf(t_out, (B0[a] - cam.eye[a]) / d[a]);
                }
                int kn = k + 1;
                const int kp = render_propose(cam, t_out, k);
                if (kp > k) {
                    float q[3];
                    rdef::point_at(cam, d, rdef::sample_t(cam, kp), q);
                    if (q[0] >= B0[0] && q[0] < B1[0] && q[1] >= B0[1] && q[1] < B1[1] && q[2] >= B0[2] && q[2] < B1[2]) kn = kp + 1;
                }
                k = kn;
                continue;
            }
            float v[8];
            render_corners(g, tv, flags, c, v);
            const float v1 = rdef::trilinear(v, f);
            if (v1 < 0.0f) {
                hit = true;
                if (k == 0) t = tk;
                else {
                    const float t0 = rdef::sample_t(cam, k - 1);
                    float p0[3];
                    rdef::point_at(cam, d, t0, p0);
                    t = rdef::hit_time(t0, tk, render_value(g, tv, flags, p0), v1);
                }
                break;
            }
            ++k;
        }
        if (hit) {
            float ph[3];
            rdef::point_at(cam, d, t, ph);
            if (rdef::in_bounds(ph, g.lo, g.hi)) {
                int c[3];
                float f[3], v[8];
                rdef::cell_of(ph, c, f);
                render_corners(g, tv, flags, c, v);
                rdef::normal_of(v, f, n);
            }
        }
    }
    const unsigned long long hb = __ballot(hit);
    if (lane == 0 && hb) atomicAdd(hits, (unsigned)__popcll(hb));
    if (!mine) return;
    const size_t at = (size_t)j * cam.width + i;
    if (rgb) {
        unsigned char c3[3] = {sh.background[0], sh.background[1], sh.background[2]};
        if (hit) rdef::shade(sh, n, d, c3);
        rgb[3 * at] = c3[0], rgb[3 * at + 1] = c3[1], rgb[3 * at + 2] = c3[2];
    }
    if (depth) depth[at] = t;
    if (normals) normals[3 * at] = n[0], normals[3 * at + 1] = n[1], normals[3 * at + 2] = n[2];
}

// neg[leaves of the range], occ[(ext_leaves + 31) / 32 words]; r.any == 0: neither is touched, every pixel is a miss.  hits: the
// record's first word, zeroed by the caller on the same stream.  rgb / depth / normals: nullptr for a part not asked for
void launch_render(hipStream_t st, const RenderGeom& r, const fluid_camera_t& cam, const fluid_shade_t& sh, const float* tv, const int* flags,
                   unsigned char* neg, unsigned* occ, unsigned* hits, unsigned char* rgb, float* depth, float* normals)
{
    if (r.any) {
        const long leaves = r.g.leaves(), words = (r.ext_leaves() + 31) / 32;
        hipLaunchKernelGGL(k_render_neg, dim3((unsigned)((leaves + 3) / 4)), dim3(256), 0, st, leaves, tv, flags, neg);
        hipLaunchKernelGGL(k_render_occ, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, r, (const unsigned char*)neg, occ);
    }
    hipLaunchKernelGGL(k_render_march, dim3((unsigned)((cam.width + 15) / 16), (unsigned)((cam.height + 15) / 16)), dim3(256), 0, st, r, cam, sh, tv, flags,
                       (const unsigned*)occ, hits, rgb, depth, normals);
}

}  // namespace fl
