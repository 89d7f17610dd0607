// Narrow-band level set of the particles for gfx950 (wave64): the signed distance to the union of spheres of radius R around the
// particles, clipped to a band of half width w, as the leaves of OpenVDB's tree (include/fluid_hip.h, "liquid surface";
// fluid_sdf.hip).  The value of a voxel is a function of the MINIMUM squared distance over the particles, so no order is involved:
//   bin      the particles (of a decomposed handle: the live ones, k_sdf_bbox<true> / k_sdf_count<true>) whose base cell round(p)
//            lies in the grid are counted per cell of their bounding box (integer atomics
//            hand out a place inside the cell: which place does not matter to a minimum), the counts are scanned, the positions
//            are scattered into cell order (z fastest), all in scratch of the snapshot's own;
//   search   one 512-thread block per leaf of the box dilated by 4 cells: the cell starts of the leaf's 16^3 neighbourhood go to
//            LDS (17 per z row: 17 KB), a leaf with no particle in reach leaves at once, a thread owns one voxel and walks the
//            Chebyshev rings of cells around it;
//   pack     the listed leaves' values, masks and origins in ascending order (exclusive scan of the flags; masks by ballot).
// Attributes (include/fluid_hip.h, "liquid surface, attributes"): template flags on scatter, search and pack carry the closest
// particle's id and velocity along; the plain instantiations are the code they were.
// Ring stop.  A particle whose base cell is k + 1 cells away on some axis has |c - p| >= k + 0.5 on that axis, exactly
// (|p - round(p)| <= 0.5).  k + 0.5 and its square are floats, every rounding below is monotone and every addend non-negative, so
// the particle's x2y2z2 AS COMPUTED is >= (k + 0.5)^2: once the minimum so far is <= that, no ring further out can lower it, and
// no margin for the three narrowings is needed (the walk asks for strictly below all the same).  It also ends once
// (k + 0.5)^2 >= max2 (whatever is further out is outside the band) or the minimum is <= min2 (the voxel is -bg whatever follows).
// R + w <= 4 bounds max2 by 16 < 4.5^2: ring 4 is the last.
// Arithmetic of the distance: include/fluid_hip.h; differences and squares in double, one narrowing to float per axis, no FMA
// (-ffp-contract=off), sqrt correctly rounded.
#include "common.h"

#include <limits.h>

namespace fl {

// base cell of a particle, compared as doubles (NaN and far-off positions are in no cell of the grid)
__device__ __forceinline__ bool sdf_cell(double px, double py, double pz, int lo, int hi, int& cx, int& cy, int& cz)
{
    const double rx = round(px), ry = round(py), rz = round(pz);
    if (!(rx >= (double)lo && rx <= (double)hi && ry >= (double)lo && ry <= (double)hi && rz >= (double)lo && rz <= (double)hi)) return false;
    cx = (int)rx, cy = (int)ry, cz = (int)rz;
    return true;
}

__global__ void k_sdf_box_init(int* __restrict__ box)
{
    if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
}

// box[0..2] = min, box[3..5] = max of the counted particles' base cells (integer min / max: order-free)
// LIVE (here and in k_sdf_count): the arrays of a decomposed handle, where an entry with pid == PID_DEAD is a ghost that was served
// or a particle a sink removed, with a stale position: it is in no cell.  The one-GPU form never reads pid.
template <bool LIVE>
__global__ __launch_bounds__(256) void k_sdf_bbox(long n, const double* __restrict__ px, const double* __restrict__ py,
                                                  const double* __restrict__ pz, int lo, int hi, int* __restrict__ box,
                                                  const uint32_t* __restrict__ pid)
{
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        int c[3];
        if (LIVE && pid[i] == PID_DEAD) continue;
        if (!sdf_cell(px[i], py[i], pz[i], lo, hi, c[0], c[1], c[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = c[a] < mn[a] ? c[a] : mn[a];
            mx[a] = c[a] > mx[a] ? c[a] : mx[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int u = __shfl_down(mn[a], o, 64), v = __shfl_down(mx[a], o, 64);
            mn[a] = u < mn[a] ? u : mn[a];
            mx[a] = v > mx[a] ? v : mx[a];
        }
    }
    if ((threadIdx.x & 63) == 0 && mx[0] >= mn[0]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&box[a], mn[a]);
            atomicMax(&box[3 + a], mx[a]);
        }
    }
}

__device__ __forceinline__ long sdf_box_index(const SdfGeom& g, int cx, int cy, int cz)
{
    return ((long)(cx - g.bx0) * g.bny + (cy - g.by0)) * g.bnz + (cz - g.bz0);
}

// cnt[cell]++ over the box; place[i] = the particle's place inside its cell (-1: not counted, and k_sdf_scatter passes it over:
// a dead entry is never scattered)
template <bool LIVE>
__global__ __launch_bounds__(256) void k_sdf_count(long n, const double* __restrict__ px, const double* __restrict__ py,
                                                   const double* __restrict__ pz, SdfGeom g, int* __restrict__ cnt, int* __restrict__ place,
                                                   const uint32_t* __restrict__ pid)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (LIVE && pid[i] == PID_DEAD) {
        place[i] = -1;
        return;
    }
    int cx, cy, cz;
    place[i] = sdf_cell(px[i], py[i], pz[i], g.lo, g.hi, cx, cy, cz) ? atomicAdd(&cnt[sdf_box_index(g, cx, cy, cz)], 1) : -1;
}

// ATTR: ssrc[d] = i as well, the index in the live arrays of the particle at sorted position d (after a step the live arrays are
// in the step's sort order, not in id order: the attribute search goes through ssrc to pid and the velocities)
template <bool ATTR>
__global__ __launch_bounds__(256) void k_sdf_scatter(long n, const double* __restrict__ px, const double* __restrict__ py,
                                                     const double* __restrict__ pz, SdfGeom g, const int* __restrict__ start,
                                                     const int* __restrict__ place, double* __restrict__ sx, double* __restrict__ sy,
                                                     double* __restrict__ sz, int* __restrict__ ssrc)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || place[i] < 0) return;
    const double x = px[i], y = py[i], z = pz[i];
    int cx, cy, cz;
    sdf_cell(x, y, z, g.lo, g.hi, cx, cy, cz);
    const long d = (long)start[sdf_box_index(g, cx, cy, cz)] + place[i];
    sx[d] = x, sy[d] = y, sz[d] = z;
    if (ATTR) ssrc[d] = (int)i;
}

__device__ __forceinline__ float sdf_dist2(int vx, int vy, int vz, double x, double y, double z)
{
    const double ax = (double)vx - x, ay = (double)vy - y, az = (double)vz - z;
    const float x2 = (float)(ax * ax);
    const float x2y2 = (float)((double)x2 + ay * ay);
    return (float)((double)x2y2 + az * az);
}

// One block per leaf j of the range, thread t = the voxel's offset in the leaf ((x&7)*8 + (y&7))*8 + (z&7): wave x holds the
// leaf's x plane, its ballot is word x of the mask.  S[(lx * 16 + ly) * 17 + lz] = start of cell (o - 4 + (lx, ly, lz)) in the
// sorted arrays, lz = 16 being the end of the row's last cell; rows and cells outside the particles' box are empty (equal starts).
// tv / tm: 512 values and 8 mask words per leaf of the range; flags[j] = the leaf is listed.  VISITS: visits[j] = cells looked at
// by the leaf's voxels (a figure for tools/sdf_cost.py; the plain kernel does not count).
// ARGMIN ("liquid surface, attributes"): the sorted position of the particle that gave m travels with m.  A strictly smaller x2
// replaces it; an equal one (rare) loads both ids through ssrc -> pid and keeps the smaller, so the winner is the smallest id among
// the particles at the minimum whatever order the walk meets them in.  The ring stop asks for m strictly below (k + 0.5)^2 <= every
// x2 further out, so no particle tied with the minimum is left unvisited for a voxel that ends up active.  m itself is updated by
// the same fminf: values and masks are those of the plain kernel.  Every thread of a flagged leaf writes tid (512 per leaf) and
// tvel ([leaf][axis][512]): the winner's id and narrowed velocity where the voxel is active, NO_ID / +0 elsewhere.  A block that
// leaves early writes the flag alone: its tid / tvel are stale and never read.
// DIST2 ("liquid surface, attributes (decomposed runs)"; with ARGMIN only): every thread of a flagged leaf also writes tmin (512 per
// leaf), m itself where the voxel is active and +inf elsewhere: what a host merge of rank records decides on.  m is in a register at
// that point: one more coalesced 4-byte store per thread, nothing else differs from the ARGMIN form.
__device__ __forceinline__ void sdf_visit(float& m, float x2) { m = fminf(m, x2); }
__device__ __forceinline__ void sdf_visit_arg(float& m, int& best, float x2, int p, const int* __restrict__ ssrc, const uint32_t* __restrict__ pid)
{
    if (x2 < m) best = p;
    else if (x2 == m && best >= 0 && pid[ssrc[p]] < pid[ssrc[best]]) best = p;
    m = fminf(m, x2);
}

template <bool VISITS, bool ARGMIN, bool DIST2 = false>
__global__ __launch_bounds__(512) void k_sdf_search(SdfGeom g, const int* __restrict__ start, const double* __restrict__ sx,
                                                    const double* __restrict__ sy, const double* __restrict__ sz, float* __restrict__ tv,
                                                    unsigned long long* __restrict__ tm, int* __restrict__ flags, unsigned* __restrict__ visits,
                                                    const int* __restrict__ ssrc, const uint32_t* __restrict__ pid,
                                                    const double* __restrict__ pvx, const double* __restrict__ pvy,
                                                    const double* __restrict__ pvz, uint32_t* __restrict__ tid, float* __restrict__ tvel,
                                                    float* __restrict__ tmin)
{
    __shared__ int S[16 * 16 * 17];
    __shared__ unsigned vis[8];
    const int t = threadIdx.x;
    const long j = blockIdx.x;
    const int jz = (int)(j % g.nl[2]), jy = (int)((j / g.nl[2]) % g.nl[1]), jx = (int)(j / ((long)g.nl[1] * g.nl[2]));
    const int ox = g.L0 + 8 * (g.l0[0] + jx), oy = g.L0 + 8 * (g.l0[1] + jy), oz = g.L0 + 8 * (g.l0[2] + jz);
    for (int i = t; i < 16 * 16 * 17; i += 512) {
        const int k = i % 17, r = i / 17, ly = r & 15, lx = r >> 4;
        const int cx = ox - 4 + lx - g.bx0, cy = oy - 4 + ly - g.by0;
        int v = 0;
        if (cx >= 0 && cx < g.bnx && cy >= 0 && cy < g.bny) {
            int zc = oz - 4 + k - g.bz0;
            zc = zc < 0 ? 0 : (zc > g.bnz ? g.bnz : zc);
            v = start[((long)cx * g.bny + cy) * g.bnz + zc];
        }
        S[i] = v;
    }
    __syncthreads();
    const int any = __syncthreads_or(t < 256 && S[t * 17 + 16] != S[t * 17]);
    if (!any) {   // no particle within 4 cells of the leaf: every voxel is inactive +bg
        if (t == 0) {
            flags[j] = 0;
            if (VISITS) visits[j] = 0;
        }
        return;
    }
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const int vx = ox + x, vy = oy + y, vz = oz + z;
    const bool in = vx >= g.lo && vx <= g.hi && vy >= g.lo && vy <= g.hi && vz >= g.lo && vz <= g.hi;
    float m = INFINITY;
    int best = -1;
    unsigned nvis = 0;
    if (in) {
        const int zc = z + 4;
        for (int k = 0; k <= 4; ++k) {
            for (int dx = -k; dx <= k; ++dx)
                for (int dy = -k; dy <= k; ++dy) {
                    const int row = ((x + 4 + dx) * 16 + (y + 4 + dy)) * 17 + zc;
                    const bool shell = dx == -k || dx == k || dy == -k || dy == k;   // the whole z run belongs to ring k
                    // the cells of a z run are contiguous in the sorted arrays: one range; else the run's two end cells
                    const int b0 = S[row - k], e0 = shell ? S[row + k + 1] : S[row - k + 1];
                    for (int p = b0; p < e0; ++p) {
                        const float x2 = sdf_dist2(vx, vy, vz, sx[p], sy[p], sz[p]);
                        if (ARGMIN) sdf_visit_arg(m, best, x2, p, ssrc, pid);
                        else sdf_visit(m, x2);
                    }
                    if (!shell) {
                        const int b1 = S[row + k], e1 = S[row + k + 1];
                        for (int p = b1; p < e1; ++p) {
                            const float x2 = sdf_dist2(vx, vy, vz, sx[p], sy[p], sz[p]);
                            if (ARGMIN) sdf_visit_arg(m, best, x2, p, ssrc, pid);
                            else sdf_visit(m, x2);
                        }
                    }
                    if (VISITS) nvis += shell ? 2 * k + 1 : 2;
                }
            const float T = ((float)k + 0.5f) * ((float)k + 0.5f);
            if (m < T || T >= g.max2 || m <= g.min2) break;
        }
    }
    float val = g.bg;
    bool act = false;
    if (in && m < g.max2) {
        if (m <= g.min2) {
            val = -g.bg;
        } else {
            // sqrtf is the IEEE root (-fhip-fp32-correctly-rounded-divide-sqrt, Makefile); __fsqrt_rn is the 1-ulp native one
            const float d = g.dxf * (sqrtf(m) - g.R);
            if (d < g.bg) val = d, act = true;
        }
    }
    tv[j * 512 + t] = val;
    if (ARGMIN) {
        uint32_t id = 0xffffffffu;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        if (act && best >= 0) {   // (an active voxel has m < inf, so a winner)
            const int src = ssrc[best];
            id = pid[src];
            a0 = (float)pvx[src], a1 = (float)pvy[src], a2 = (float)pvz[src];
        }
        tid[j * 512 + t] = id;
        float* tw = tvel + j * 1536 + t;
        tw[0] = a0, tw[512] = a1, tw[1024] = a2;
        if (DIST2) tmin[j * 512 + t] = act ? m : INFINITY;
    }
    const unsigned long long b = __ballot(act);
    if ((t & 63) == 0) tm[j * 8 + x] = b;
    const int listed = __syncthreads_or(in && (act || val != g.bg));
    if (t == 0) flags[j] = listed ? 1 : 0;
    if (VISITS) {
        nvis = wave_sum(nvis);
        if ((t & 63) == 0) vis[x] = nvis;
        __syncthreads();
        if (t == 0) visits[j] = vis[0] + vis[1] + vis[2] + vis[3] + vis[4] + vis[5] + vis[6] + vis[7];
    }
}

// One wave per leaf of the range; the waves of unlisted leaves leave at once.  slot[j] = the record's place in the list.
// ATTR: the leaf's 512 ids and 3 x 512 velocities as well, in 16-byte copies (every base is a multiple of 2048 bytes from hipMalloc's).
// DIST2 (with ATTR only): and its 512 squared distances, two more 16-byte copies per lane.
template <bool ATTR, bool DIST2 = false>
__global__ __launch_bounds__(256) void k_sdf_pack(SdfGeom g, long nrange, const int* __restrict__ flags, const int* __restrict__ slot,
                                                  const float* __restrict__ tv, const unsigned long long* __restrict__ tm,
                                                  float* __restrict__ values, unsigned long long* __restrict__ active, int* __restrict__ origin,
                                                  const uint32_t* __restrict__ tid, const float* __restrict__ tvel, uint32_t* __restrict__ ids,
                                                  float* __restrict__ vel, const float* __restrict__ tmin, float* __restrict__ dist2)
{
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= nrange || !flags[j]) return;
    const int lane = threadIdx.x & 63;
    const int jz = (int)(j % g.nl[2]), jy = (int)((j / g.nl[2]) % g.nl[1]), jx = (int)(j / ((long)g.nl[1] * g.nl[2]));
    const long s = slot[j];
    const float4* src = (const float4*)(tv + j * 512 + lane * 8);
    float4* dst = (float4*)(values + s * 512 + lane * 8);   // 32-byte aligned: both bases are hipMalloc's
    dst[0] = src[0];
    dst[1] = src[1];
    if (lane < 8) active[s * 8 + lane] = tm[j * 8 + lane];
    if (lane < 3) origin[s * 3 + lane] = g.L0 + 8 * (g.l0[lane] + (lane == 0 ? jx : lane == 1 ? jy : jz));
    if (ATTR) {
        const uint4* is = (const uint4*)(tid + j * 512);
        uint4* id = (uint4*)(ids + s * 512);
        id[lane] = is[lane];
        id[lane + 64] = is[lane + 64];
        const float4* vs = (const float4*)(tvel + j * 1536);
        float4* vd = (float4*)(vel + s * 1536);
#pragma unroll
        for (int k = 0; k < 6; ++k) vd[lane + 64 * k] = vs[lane + 64 * k];
        if (DIST2) {
            const float4* ms = (const float4*)(tmin + j * 512);
            float4* md = (float4*)(dist2 + s * 512);
            md[lane] = ms[lane];
            md[lane + 64] = ms[lane + 64];
        }
    }
}

void launch_sdf_bbox(hipStream_t st, long n, Particles p, int lo, int hi, int* box, bool live)
{
    hipLaunchKernelGGL(k_sdf_box_init, dim3(1), dim3(64), 0, st, box);
    if (n <= 0) return;
    const long nb = (n + 255) / 256;
    const dim3 grid((unsigned)(nb < 2048 ? nb : 2048));
    if (live) hipLaunchKernelGGL(k_sdf_bbox<true>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, lo, hi, box, p.pid);
    else hipLaunchKernelGGL(k_sdf_bbox<false>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, lo, hi, box, (const uint32_t*)nullptr);
}

void launch_sdf_count(hipStream_t st, long n, Particles p, const SdfGeom& g, int* cnt, int* place, bool live)
{
    const dim3 grid((unsigned)((n + 255) / 256));
    if (live) hipLaunchKernelGGL(k_sdf_count<true>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, g, cnt, place, p.pid);
    else hipLaunchKernelGGL(k_sdf_count<false>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, g, cnt, place, (const uint32_t*)nullptr);
}

void launch_sdf_scatter(hipStream_t st, long n, Particles p, const SdfGeom& g, const int* start, const int* place, double* sx, double* sy,
                        double* sz, int* ssrc)
{
    const dim3 grid((unsigned)((n + 255) / 256));
    if (ssrc) hipLaunchKernelGGL(k_sdf_scatter<true>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, g, start, place, sx, sy, sz, ssrc);
    else hipLaunchKernelGGL(k_sdf_scatter<false>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, g, start, place, sx, sy, sz, ssrc);
}

void launch_sdf_search(hipStream_t st, const SdfGeom& g, const int* start, const double* sx, const double* sy, const double* sz, float* tv,
                       uint64_t* tm, int* flags, unsigned* visits)
{
    const unsigned nb = (unsigned)g.leaves();
    const int* ns = nullptr;
    const uint32_t* nu = nullptr;
    const double* nd = nullptr;
    if (visits)
        hipLaunchKernelGGL((k_sdf_search<true, false>), dim3(nb), dim3(512), 0, st, g, start, sx, sy, sz, tv, (unsigned long long*)tm, flags, visits, ns,
                           nu, nd, nd, nd, (uint32_t*)nullptr, (float*)nullptr, (float*)nullptr);
    else
        hipLaunchKernelGGL((k_sdf_search<false, false>), dim3(nb), dim3(512), 0, st, g, start, sx, sy, sz, tv, (unsigned long long*)tm, flags, visits, ns,
                           nu, nd, nd, nd, (uint32_t*)nullptr, (float*)nullptr, (float*)nullptr);
}

void launch_sdf_search_attr(hipStream_t st, const SdfGeom& g, const int* start, const double* sx, const double* sy, const double* sz, float* tv,
                            uint64_t* tm, int* flags, const int* ssrc, Particles p, uint32_t* tid, float* tvel, float* tmin)
{
    if (tmin)
        hipLaunchKernelGGL((k_sdf_search<false, true, true>), dim3((unsigned)g.leaves()), dim3(512), 0, st, g, start, sx, sy, sz, tv,
                           (unsigned long long*)tm, flags, (unsigned*)nullptr, ssrc, (const uint32_t*)p.pid, (const double*)p.vx, (const double*)p.vy,
                           (const double*)p.vz, tid, tvel, tmin);
    else
        hipLaunchKernelGGL((k_sdf_search<false, true>), dim3((unsigned)g.leaves()), dim3(512), 0, st, g, start, sx, sy, sz, tv, (unsigned long long*)tm,
                           flags, (unsigned*)nullptr, ssrc, (const uint32_t*)p.pid, (const double*)p.vx, (const double*)p.vy, (const double*)p.vz, tid, tvel,
                           (float*)nullptr);
}

void launch_sdf_pack(hipStream_t st, const SdfGeom& g, const int* flags, const int* slot, const float* tv, const uint64_t* tm, float* values,
                     uint64_t* active, int* origin)
{
    const long nrange = g.leaves();
    hipLaunchKernelGGL(k_sdf_pack<false>, dim3((unsigned)((nrange + 3) / 4)), dim3(256), 0, st, g, nrange, flags, slot, tv, (const unsigned long long*)tm,
                       values, (unsigned long long*)active, origin, (const uint32_t*)nullptr, (const float*)nullptr, (uint32_t*)nullptr, (float*)nullptr,
                       (const float*)nullptr, (float*)nullptr);
}

void launch_sdf_pack_attr(hipStream_t st, const SdfGeom& g, const int* flags, const int* slot, const float* tv, const uint64_t* tm, float* values,
                          uint64_t* active, int* origin, const uint32_t* tid, const float* tvel, uint32_t* ids, float* vel, const float* tmin, float* dist2)
{
    const long nrange = g.leaves();
    if (tmin)
        hipLaunchKernelGGL((k_sdf_pack<true, true>), dim3((unsigned)((nrange + 3) / 4)), dim3(256), 0, st, g, nrange, flags, slot, tv,
                           (const unsigned long long*)tm, values, (unsigned long long*)active, origin, tid, tvel, ids, vel, tmin, dist2);
    else
        hipLaunchKernelGGL((k_sdf_pack<true>), dim3((unsigned)((nrange + 3) / 4)), dim3(256), 0, st, g, nrange, flags, slot, tv,
                           (const unsigned long long*)tm, values, (unsigned long long*)active, origin, tid, tvel, ids, vel, (const float*)nullptr,
                           (float*)nullptr);
}

}  // namespace fl
