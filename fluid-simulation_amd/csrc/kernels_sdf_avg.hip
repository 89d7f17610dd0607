// The search of the averaged-position surface for gfx950 (wave64): include/fluid_hip.h, "liquid surface, averaged positions";
// arithmetic in sdf_avg_def.h.  It takes the place of k_sdf_search (kernels_sdf.hip) behind the same bin, scan and scatter and in
// front of the same filters, pack, mesh and ray caster: same SdfGeom, same cell starts in LDS, same early exit of a leaf out of
// reach, same tv / tm / flags.  Only the walk and the finish differ.
// The walk.  A voxel's value is a function of a minimum and of four integer sums over EVERY particle within hf, so no lane can stop
// at a ring of its own, and a sum does not care about order: a wave (one x plane of the leaf) walks the z runs of its planes' cell
// neighbourhood in unison.  For ring K (adef::last_ring: the last ring that can weigh or lie in the band) that is the rows
// (x - K .. x + K) x (oy - K .. oy + 7 + K), each one contiguous range of the sorted arrays (cells oz - K .. oz + 7 + K, z fastest).
// A range goes through the wave's own 1.5 KB of LDS in chunks of 64 particles: lane i loads particle i (coalesced), forms what the
// whole wave shares (the x term of the squared distance and O_x: every lane of the wave has the same vx) and stores y, z and those
// two; then every lane reads the 64 back, one at a time, as broadcasts (one 16-byte and one 8-byte read per particle), finishes
// x2y2z2 exactly as adef::dist2 does, lowers m and, after the float test x2 < h2, adds the weight and the three products.  The waves
// of a block do not wait for each other between the starts and the flag: the LDS of a wave is written and read by that wave alone,
// whose LDS operations complete in order; the fences at wavefront scope keep the compiler from moving them across each other.
// A lane meets particles it cannot use (a wave's rows span 16 cells in y and z where a voxel reaches 9): 3.2 times the particles
// of a walk per lane at K = 4, each rejected after the two remaining axes of the distance.  What that costs beside the spheres'
// search: profiles/avg/NOTES.md.
// A plane whose in-grid voxels all have m <= min2 (they are inactive -bg whatever follows) stops; x planes are taken from the
// voxel's own outwards so that a deep interior gets there early.
// RECORD ("liquid surface, averaged positions (decomposed runs)"): same walk, LDS and early stops; the finish writes what a merge
// over ranks needs in place of the value: the canonical dist2 (m inside (min2, reach2), +0 at or below min2, +inf elsewhere) where
// tv would go, and the four sums as four planes of 512 uint64 per leaf (a wave's 64 stores of a plane are 512 contiguous bytes),
// zero wherever dist2 is +0 or +inf.  The leaf's flag is m < reach2 over its in-grid voxels, reach2 = max(max2, h2): a particle
// can weigh on a voxel that lies outside its own band.  No tv / tm.  k_sdf_pack_avg lists the flagged leaves' records.
#include "common.h"
#include "sdf_avg_def.h"

namespace fl {

// RECORD: tv is the range's dist2 (512 per leaf) and tm its sums ([leaf][4][512])
template <bool RECORD>
__global__ __launch_bounds__(512) void k_sdf_search_avg(SdfGeom g, adef::Consts hc, int K, const int* __restrict__ start,
                                                        const double* __restrict__ sx, const double* __restrict__ sy,
                                                        const double* __restrict__ sz, float* __restrict__ tv,
                                                        unsigned long long* __restrict__ tm, int* __restrict__ flags)
{
    __shared__ int S[16 * 16 * 17];
    __shared__ double2 Pyz[8][64];   // per wave: y, z of the chunk's particles
    __shared__ int2 Pxo[8][64];      // and the x term of x2y2z2 (float bits) and O_x
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
        if (t == 0) flags[j] = 0;
        return;
    }
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7, lane = t & 63;
    const int vx = ox + x, vy = oy + y, vz = oz + z;
    const bool in = vx >= g.lo && vx <= g.hi && vy >= g.lo && vy <= g.hi && vz >= g.lo && vz <= g.hi;
    float m = INFINITY;
    adef::Sums sum;
    // every lane walks, in or out of the grid: the wave stays whole, and a voxel outside the grid is written as +bg below
    for (int q = 0; q <= 2 * K; ++q) {
        const int lx = x + 4 + ((q & 1) ? -((q + 1) >> 1) : (q >> 1));   // 0, -1, +1, -2, +2, ...
        for (int ly = 4 - K; ly <= 11 + K; ++ly) {
            const int row = (lx * 16 + ly) * 17;
            const int b = __builtin_amdgcn_readfirstlane(S[row + 4 - K]), e = __builtin_amdgcn_readfirstlane(S[row + 12 + K]);
            for (int p0 = b; p0 < e; p0 += 64) {
                const int cnt = e - p0 < 64 ? e - p0 : 64;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the reads of the chunk before are done with
                if (lane < cnt) {
                    const double px = sx[p0 + lane];
                    Pyz[x][lane] = make_double2(sy[p0 + lane], sz[p0 + lane]);
                    Pxo[x][lane] = make_int2(__float_as_int(adef::dist2_x((double)vx - px)), adef::offset(px, vx));
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                for (int i = 0; i < cnt; ++i) {
                    const double2 yz = Pyz[x][i];
                    const int2 xo = Pxo[x][i];
                    const float x2 = adef::dist2_yz(__int_as_float(xo.x), vy, vz, yz.x, yz.y);
                    m = fminf(m, x2);
                    if (x2 < hc.h2) adef::add(sum, adef::weight(x2, hc), xo.y, adef::offset(yz.x, vy), adef::offset(yz.y, vz));
                }
            }
        }
        if (__all(!in || m <= g.min2)) break;
    }
    if (RECORD) {
        const float reach2 = fmaxf(g.max2, hc.h2);
        const bool reached = in && m < reach2;
        const bool keep = reached && m > g.min2;   // the sums of every other voxel are never read: 0, so that the record is canonical
        tv[j * 512 + t] = keep ? m : (reached ? 0.0f : INFINITY);
        unsigned long long* sums = tm + j * 2048 + t;
        sums[0] = keep ? sum.w : 0ull;
        sums[512] = keep ? sum.x : 0ull;
        sums[1024] = keep ? sum.y : 0ull;
        sums[1536] = keep ? sum.z : 0ull;
        const int listed = __syncthreads_or(reached);
        if (t == 0) flags[j] = listed ? 1 : 0;
        return;
    }
    float val = g.bg;
    bool act = false;
    if (in) adef::finish(m, sum, true, g.R, g.dxf, g.bg, g.max2, g.min2, val, act);
    tv[j * 512 + t] = val;
    const unsigned long long bal = __ballot(act);
    if (lane == 0) tm[j * 8 + x] = bal;
    const int listed = __syncthreads_or(in && (act || val != g.bg));
    if (t == 0) flags[j] = listed ? 1 : 0;
}

void launch_sdf_search_avg(hipStream_t st, const SdfGeom& g, float h2, float ih2, const int* start, const double* sx, const double* sy,
                           const double* sz, float* tv, uint64_t* tm, int* flags)
{
    adef::Consts hc;
    hc.h2 = h2, hc.ih2 = ih2;
    hipLaunchKernelGGL(k_sdf_search_avg<false>, dim3((unsigned)g.leaves()), dim3(512), 0, st, g, hc, adef::last_ring(h2, g.max2), start, sx, sy, sz, tv,
                       (unsigned long long*)tm, flags);
}

void launch_sdf_search_avg_record(hipStream_t st, const SdfGeom& g, float h2, float ih2, const int* start, const double* sx, const double* sy,
                                  const double* sz, float* tdist2, uint64_t* tsum, int* flags)
{
    adef::Consts hc;
    hc.h2 = h2, hc.ih2 = ih2;
    hipLaunchKernelGGL(k_sdf_search_avg<true>, dim3((unsigned)g.leaves()), dim3(512), 0, st, g, hc, adef::last_ring(h2, g.max2), start, sx, sy, sz, tdist2,
                       (unsigned long long*)tsum, flags);
}

// One wave per leaf of the range, as k_sdf_pack (kernels_sdf.hip); the waves of unlisted leaves leave at once.  The leaf's 2048 bytes
// of dist2 and 16384 bytes of sums go to slot[j] of the record in 16-byte copies (every base is a multiple of 2048 bytes from
// hipMalloc's), its origin behind them.
__global__ __launch_bounds__(256) void k_sdf_pack_avg(SdfGeom g, long nrange, const int* __restrict__ flags, const int* __restrict__ slot,
                                                      const float* __restrict__ tdist2, const unsigned long long* __restrict__ tsum,
                                                      float* __restrict__ dist2, unsigned long long* __restrict__ sums, int* __restrict__ origin)
{
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= nrange || !flags[j]) return;
    const int lane = threadIdx.x & 63;
    const int jz = (int)(j % g.nl[2]), jy = (int)((j / g.nl[2]) % g.nl[1]), jx = (int)(j / ((long)g.nl[1] * g.nl[2]));
    const long s = slot[j];
    const float4* ms = (const float4*)(tdist2 + j * 512);
    float4* md = (float4*)(dist2 + s * 512);
    md[lane] = ms[lane];
    md[lane + 64] = ms[lane + 64];
    const uint4* ss = (const uint4*)(tsum + j * 2048);
    uint4* sd = (uint4*)(sums + s * 2048);
#pragma unroll
    for (int k = 0; k < 16; ++k) sd[lane + 64 * k] = ss[lane + 64 * k];
    if (lane < 3) origin[s * 3 + lane] = g.L0 + 8 * (g.l0[lane] + (lane == 0 ? jx : lane == 1 ? jy : jz));
}

void launch_sdf_pack_avg(hipStream_t st, const SdfGeom& g, const int* flags, const int* slot, const float* tdist2, const uint64_t* tsum,
                         float* dist2, uint64_t* sums, int* origin)
{
    const long nrange = g.leaves();
    hipLaunchKernelGGL(k_sdf_pack_avg, dim3((unsigned)((nrange + 3) / 4)), dim3(256), 0, st, g, nrange, flags, slot, tdist2,
                       (const unsigned long long*)tsum, dist2, (unsigned long long*)sums, origin);
}

}  // namespace fl
