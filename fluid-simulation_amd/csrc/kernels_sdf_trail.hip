// Velocity trails for gfx950 (wave64): include/fluid_hip.h, "liquid surface, velocity trails"; arithmetic in sdf_trail_def.h.
// Every live particle becomes a short chain of shrinking spheres along -velocity (its instances); the level set is the union of
// all of them.  A voxel is no longer a function of the minimum squared distance (that needs one radius), so the items of the search
// carry their radius.
//   expand   two passes over the live particles, each running tdef::next.  The first counts a particle's instances (icnt), adds
//            them to a 64-bit total and reduces the base-cell box of the instances that lie in the grid (integer min / max, as
//            k_sdf_bbox).  After the scan of icnt the second writes ix, iy, iz (double) and ir (float) at the particle's slots.
//            LIVE (as in k_sdf_bbox): the arrays of a decomposed handle, where an entry with pid == PID_DEAD has a stale position
//            and velocity: it has no instance (icnt 0, nothing to the box or the total, no slot written), and the first pass also
//            counts the live entries.  The one-GPU form never reads pid.
//   bin      k_sdf_count<false> (kernels_sdf.hip) on the instance arrays as it stands; the scatter here carries the radius.
//   search   k_sdf_search_rad, in the place of k_sdf_search: same cell starts in LDS, same early exit of a leaf out of reach, same
//            tv / tm / flags.
// The walk is k_sdf_search's, a thread per voxel with ring stops of its own.  A wave walking the z runs of its plane's neighbourhood
// in unison (k_sdf_search_avg's walk, items staged through LDS) was built and measured as well: 0.6 times the spheres' search over
// the same items in a settled pool, but 2.9 and 3.8 times in the splash and in the fresh cube, where this one takes 1.16 and 1.13
// times (profiles/trail/NOTES.md); the splash is what trails are for.
// Only the source of the items is particular to trails: the search reads (sx, sy, sz, sr) and would serve radii given per particle.
#include "common.h"
#include "sdf_trail_def.h"

#include <limits.h>

namespace fl {

// base cell of a point, compared as doubles (k_sdf_bbox's rule: NaN and far-off positions are in no cell of the grid)
__device__ __forceinline__ bool trail_cell(double px, double py, double pz, int lo, int hi, int& cx, int& cy, int& cz)
{
    const double rx = round(px), ry = round(py), rz = round(pz);
    if (!(rx >= (double)lo && rx <= (double)hi && ry >= (double)lo && ry <= (double)hi && rz >= (double)lo && rz <= (double)hi)) return false;
    cx = (int)rx, cy = (int)ry, cz = (int)rz;
    return true;
}

// small[0..5] = the empty box, small[8..9] = the 64-bit total 0, small[10..11] = the 64-bit count of live entries 0
__global__ void k_trail_init(int* __restrict__ small)
{
    if (threadIdx.x < 6) small[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
    if (threadIdx.x >= 8 && threadIdx.x < 12) small[threadIdx.x] = 0;
}

// icnt[i] = instances of particle i (1 .. max_instances), in or out of the grid; box and total as described above.  LIVE: icnt[i] = 0
// for a dead entry, and *nlive += the live entries (pid and nlive are read by that form alone)
template <bool LIVE>
__global__ __launch_bounds__(256) void k_trail_count(long n, const double* __restrict__ px, const double* __restrict__ py,
                                                     const double* __restrict__ pz, const double* __restrict__ vx,
                                                     const double* __restrict__ vy, const double* __restrict__ vz, tdef::Consts tc, int lo,
                                                     int hi, int* __restrict__ icnt, int* __restrict__ box,
                                                     unsigned long long* __restrict__ total, const uint32_t* __restrict__ pid,
                                                     unsigned long long* __restrict__ nlive)
{
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
    unsigned long long made = 0, alive = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        if (LIVE) {
            if (pid[i] == PID_DEAD) {
                icnt[i] = 0;
                continue;
            }
            ++alive;
        }
        const double p0[3] = {px[i], py[i], pz[i]};
        tdef::Trail T = tdef::trail(tc, vx[i], vy[i], vz[i]);
        int k = 0;
        do {
            int c[3];
            if (trail_cell(tdef::at(T, p0[0], 0), tdef::at(T, p0[1], 1), tdef::at(T, p0[2], 2), lo, hi, c[0], c[1], c[2])) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    mn[a] = c[a] < mn[a] ? c[a] : mn[a];
                    mx[a] = c[a] > mx[a] ? c[a] : mx[a];
                }
            }
            ++k;
        } while (k < tdef::MAX_INSTANCES && tdef::next(tc, T));
        icnt[i] = k;
        made += (unsigned long long)k;
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
    made = wave_sum(made);
    if (LIVE) alive = wave_sum(alive);
    if ((threadIdx.x & 63) == 0) {
        if (made) atomicAdd(total, made);
        if (LIVE && alive) atomicAdd(nlive, alive);
        if (mx[0] >= mn[0]) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(&box[a], mn[a]);
                atomicMax(&box[3 + a], mx[a]);
            }
        }
    }
}

// the same loop again: instance k of particle i goes to slot ioff[i] + k (k < icnt[i] by construction: the loop is the count's).
// LIVE: a dead entry has no slot (its ioff is the next live particle's) and returns before the loop, which runs once before it tests
template <bool LIVE>
__global__ __launch_bounds__(256) void k_trail_expand(long n, const double* __restrict__ px, const double* __restrict__ py,
                                                      const double* __restrict__ pz, const double* __restrict__ vx,
                                                      const double* __restrict__ vy, const double* __restrict__ vz, tdef::Consts tc,
                                                      const int* __restrict__ ioff, long cap, double* __restrict__ ix, double* __restrict__ iy,
                                                      double* __restrict__ iz, float* __restrict__ ir, const uint32_t* __restrict__ pid)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (LIVE && pid[i] == PID_DEAD) return;
    const double p0[3] = {px[i], py[i], pz[i]};
    tdef::Trail T = tdef::trail(tc, vx[i], vy[i], vz[i]);
    const long d0 = ioff[i];
    int k = 0;
    do {
        const long d = d0 + k;
        if (d >= 0 && d < cap) {   // (always: the slots are the scan of the first pass's counts)
            ix[d] = tdef::at(T, p0[0], 0), iy[d] = tdef::at(T, p0[1], 1), iz[d] = tdef::at(T, p0[2], 2);
            ir[d] = T.r;
        }
        ++k;
    } while (k < tdef::MAX_INSTANCES && tdef::next(tc, T));
}

// k_sdf_scatter with the radius beside the position
__global__ __launch_bounds__(256) void k_trail_scatter(long n, const double* __restrict__ ix, const double* __restrict__ iy,
                                                       const double* __restrict__ iz, const float* __restrict__ ir, SdfGeom g,
                                                       const int* __restrict__ start, const int* __restrict__ place, double* __restrict__ sx,
                                                       double* __restrict__ sy, double* __restrict__ sz, float* __restrict__ sr)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || place[i] < 0) return;
    const double x = ix[i], y = iy[i], z = iz[i];
    int cx, cy, cz;
    trail_cell(x, y, z, g.lo, g.hi, cx, cy, cz);
    const long d = (long)start[((long)(cx - g.bx0) * g.bny + (cy - g.by0)) * g.bnz + (cz - g.bz0)] + place[i];
    sx[d] = x, sy[d] = y, sz[d] = z;
    sr[d] = ir[i];
}

// One block per leaf j of the range, thread t = the voxel's offset in the leaf: k_sdf_search's conventions for S, tv, tm and flags,
// and its walk, a thread per voxel over the Chebyshev rings of cells around it, with the item's radius read beside its position.
// Ring stop after ring k, with h = k + 0.5: the voxel is inside; or h^2 >= max2 of R (whatever is further out is outside every band,
// since r <= R); or d < dxf * (h - R): an item further out has x2 >= h^2 as computed (kernels_sdf.hip) and r <= R, so its candidate
// dxf * (sqrtf(x2) - r) is >= that bound, every rounding being monotone.  That last stop is taken only where h^2 > min2 of R as
// well, so that no item further out can say inside (its own min2 is <= that of R).
__global__ __launch_bounds__(512) void k_sdf_search_rad(SdfGeom g, const int* __restrict__ start, const double* __restrict__ sx,
                                                        const double* __restrict__ sy, const double* __restrict__ sz,
                                                        const float* __restrict__ sr, float* __restrict__ tv,
                                                        unsigned long long* __restrict__ tm, int* __restrict__ flags)
{
    __shared__ int S[16 * 16 * 17];
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
    if (!any) {
        if (t == 0) flags[j] = 0;
        return;
    }
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const int vx = ox + x, vy = oy + y, vz = oz + z;
    const bool in = vx >= g.lo && vx <= g.hi && vy >= g.lo && vy <= g.hi && vz >= g.lo && vz <= g.hi;
    bool inside = false;
    float d = INFINITY;
    if (in) {
        const int zc = z + 4;
        for (int k = 0; k <= 4; ++k) {
            for (int dx = -k; dx <= k; ++dx)
                for (int dy = -k; dy <= k; ++dy) {
                    const int row = ((x + 4 + dx) * 16 + (y + 4 + dy)) * 17 + zc;
                    const bool shell = dx == -k || dx == k || dy == -k || dy == k;   // the whole z run belongs to ring k
                    const int b0 = S[row - k], e0 = shell ? S[row + k + 1] : S[row - k + 1];
                    for (int p = b0; p < e0; ++p) {
                        const tdef::Ball bl = tdef::ball(sr[p], g.w);
                        tdef::visit(inside, d, tdef::dist2(vx, vy, vz, sx[p], sy[p], sz[p]), bl.r, bl.max2, bl.min2, g.dxf);
                    }
                    if (!shell) {
                        const int b1 = S[row + k], e1 = S[row + k + 1];
                        for (int p = b1; p < e1; ++p) {
                            const tdef::Ball bl = tdef::ball(sr[p], g.w);
                            tdef::visit(inside, d, tdef::dist2(vx, vy, vz, sx[p], sy[p], sz[p]), bl.r, bl.max2, bl.min2, g.dxf);
                        }
                    }
                }
            const float h = (float)k + 0.5f;
            if (inside || h * h >= g.max2 || (h * h > g.min2 && d < g.dxf * (h - g.R))) break;
        }
    }
    float val = g.bg;
    bool act = false;
    if (in) tdef::finish(inside, d, g.bg, val, act);
    tv[j * 512 + t] = val;
    const unsigned long long bal = __ballot(act);
    if ((t & 63) == 0) tm[j * 8 + x] = bal;
    const int listed = __syncthreads_or(in && (act || val != g.bg));
    if (t == 0) flags[j] = listed ? 1 : 0;
}

void launch_sdf_search_rad(hipStream_t st, const SdfGeom& g, const int* start, const double* sx, const double* sy, const double* sz,
                           const float* sr, float* tv, uint64_t* tm, int* flags)
{
    hipLaunchKernelGGL(k_sdf_search_rad, dim3((unsigned)g.leaves()), dim3(512), 0, st, g, start, sx, sy, sz, sr, tv, (unsigned long long*)tm, flags);
}

void launch_trail_count(hipStream_t st, long n, Particles p, const tdef::Consts& tc, int lo, int hi, int* icnt, int* small, bool live)
{
    hipLaunchKernelGGL(k_trail_init, dim3(1), dim3(64), 0, st, small);
    if (n <= 0) return;
    const long nb = (n + 255) / 256;
    const dim3 grid((unsigned)(nb < 2048 ? nb : 2048));
    unsigned long long *total = (unsigned long long*)(small + 8), *nlive = (unsigned long long*)(small + 10);
    if (live) hipLaunchKernelGGL(k_trail_count<true>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, p.vx, p.vy, p.vz, tc, lo, hi, icnt, small, total, p.pid, nlive);
    else hipLaunchKernelGGL(k_trail_count<false>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, p.vx, p.vy, p.vz, tc, lo, hi, icnt, small, total, p.pid, nlive);
}

void launch_trail_expand(hipStream_t st, long n, Particles p, const tdef::Consts& tc, const int* ioff, long cap, double* ix, double* iy,
                         double* iz, float* ir, bool live)
{
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (live) hipLaunchKernelGGL(k_trail_expand<true>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, p.vx, p.vy, p.vz, tc, ioff, cap, ix, iy, iz, ir, p.pid);
    else hipLaunchKernelGGL(k_trail_expand<false>, grid, dim3(256), 0, st, n, p.px, p.py, p.pz, p.vx, p.vy, p.vz, tc, ioff, cap, ix, iy, iz, ir, p.pid);
}

void launch_trail_scatter(hipStream_t st, long n, const double* ix, const double* iy, const double* iz, const float* ir, const SdfGeom& g,
                          const int* start, const int* place, double* sx, double* sy, double* sz, float* sr)
{
    hipLaunchKernelGGL(k_trail_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, ix, iy, iz, ir, g, start, place, sx, sy, sz, sr);
}

}  // namespace fl
