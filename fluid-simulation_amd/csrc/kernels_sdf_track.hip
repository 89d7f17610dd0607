// Renormalisation and trim of the particles' level set for gfx950 (wave64) (include/fluid_hip.h, "liquid surface, renormalised";
// fluid_sdf.hip).  The kernels work on what k_sdf_search and the box passes leave on the device; the leaves, their flags and why no
// pass clears a flag: sdf_leaf.h.
//
//   track   one launch per normalisation pass, one 512-thread block per leaf of the range, thread t = the voxel
//           ((x&7)*8 + (y&7))*8 + (z&7).  The block of an unflagged leaf leaves at once.  A flagged leaf stages its own 512 values and
//           the six 64-value faces of its face neighbours in LDS (896 floats; a 7-point stencil needs no edges or corners), +bg where
//           the neighbour is unflagged or outside the range.  Every thread writes its voxel to the OTHER buffer: an active voxel
//           tdef::track_value of its seven values (sdf_track_def.h), an inactive one its value unchanged.  Jacobi by construction.
//           TRIM (the last pass of a track): sdf_leaf.h's trim_store.
//           NORM = false: the trim alone, in place, no tile.
//   relist  list[j] = the leaf is flagged and holds anything but inactive +bg: what the scan and the pack run off after a trim.
// Arithmetic: float, no FMA (-ffp-contract=off), IEEE division and square root (-fhip-fp32-correctly-rounded-divide-sqrt).
// LDS: own value of voxel t at T[t]; face f = 2 * axis + side, in-plane position uv (y*8+z, x*8+z, x*8+y) at T[512 + 64 f + uv].
// A wave is an x plane: its x neighbours are 64 consecutive floats (own plane x -+ 1, or a whole x face), one bank each.  Along y
// and z 56 lanes read own values and 8 lanes a face row, which can share banks with them two ways; see DESIGN f13.
#include "common.h"
#include "sdf_leaf.h"
#include "sdf_track_def.h"

namespace fl {

template <bool NORM, bool TRIM, bool ATTR>
__global__ __launch_bounds__(512) void k_sdf_track(SdfGeom g, float dt, float inv, const int* __restrict__ flags, unsigned long long* tm,
                                                   const float* src, float* dst, uint32_t* __restrict__ tid, float* __restrict__ tvel)
{
    __shared__ float T[512 + 6 * 64];
    const long j = blockIdx.x;
    if (!flags[j]) return;   // (the whole block alike)
    const int t = threadIdx.x;
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const float own = src[j * 512 + t];
    if (NORM) {
        T[t] = own;
        if (t < 6 * 64) {
            // face f: the plane of the leaf at -1 (its plane 7) or +1 (its plane 0) on the axis that touches this leaf
            const int f = t >> 6, uv = t & 63, axis = f >> 1, side = f & 1;
            T[512 + t] = face_value(g, flags, src, j, axis, side, side ? 0 : 7, uv);
        }
        __syncthreads();
    }
    const bool act = leaf_active(tm, j, t);
    float val = own;
    if (NORM && act) {
        const int yz = t & 63, xz = x * 8 + z, xy = t >> 3;
        const float xm = x > 0 ? T[t - 64] : T[512 + yz], xp = x < 7 ? T[t + 64] : T[512 + 64 + yz];
        const float ym = y > 0 ? T[t - 8] : T[512 + 128 + xz], yp = y < 7 ? T[t + 8] : T[512 + 192 + xz];
        const float zm = z > 0 ? T[t - 1] : T[512 + 256 + xy], zp = z < 7 ? T[t + 1] : T[512 + 320 + xy];
        val = tdef::track_value(own, xm, xp, ym, yp, zm, zp, dt, inv);
    }
    if (TRIM) val = trim_store<ATTR>(g, j, t, x, act, val, tm, tid, tvel);   // (every lane of the wave is here: the branches above have rejoined)
    if (NORM || TRIM) dst[j * 512 + t] = val;
}

__global__ __launch_bounds__(512) void k_sdf_relist(float bg, const int* __restrict__ flags, const unsigned long long* __restrict__ tm,
                                                    const float* __restrict__ tv, int* __restrict__ list)
{
    const long j = blockIdx.x;
    const int t = threadIdx.x;
    if (!flags[j]) {   // (the whole block alike)
        if (t == 0) list[j] = 0;
        return;
    }
    const bool act = leaf_active(tm, j, t);
    const int listed = __syncthreads_or(act || tv[j * 512 + t] != bg);
    if (t == 0) list[j] = listed ? 1 : 0;
}

void launch_sdf_track(hipStream_t st, const SdfGeom& g, bool norm, bool trim, const int* flags, uint64_t* tm, const float* src, float* dst,
                      uint32_t* tid, float* tvel)
{
    const float dt = g.dxf * 0.3f, inv = 1.0f / g.dxf;
    const dim3 grid((unsigned)g.leaves()), block(512);
    unsigned long long* m = (unsigned long long*)tm;
    const bool attr = tid != nullptr;
    if (norm && !trim) hipLaunchKernelGGL((k_sdf_track<true, false, false>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
    else if (norm && attr) hipLaunchKernelGGL((k_sdf_track<true, true, true>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
    else if (norm) hipLaunchKernelGGL((k_sdf_track<true, true, false>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
    else if (trim && attr) hipLaunchKernelGGL((k_sdf_track<false, true, true>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
    else if (trim) hipLaunchKernelGGL((k_sdf_track<false, true, false>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
}

void launch_sdf_relist(hipStream_t st, const SdfGeom& g, const int* flags, const uint64_t* tm, const float* tv, int* list)
{
    hipLaunchKernelGGL(k_sdf_relist, dim3((unsigned)g.leaves()), dim3(512), 0, st, g.bg, flags, (const unsigned long long*)tm, tv, list);
}

}  // namespace fl
