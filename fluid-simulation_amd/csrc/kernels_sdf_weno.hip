// HJWENO5 renormalisation of the particles' level set for gfx950 (wave64) (include/fluid_hip.h, "liquid surface, renormalised:
// HJWENO5"; fluid_sdf.hip).  The leaves, their flags and what an unflagged leaf reads as: sdf_leaf.h.  The trim alone (no pass) and the
// relisting are scheme-independent and stay with k_sdf_track / k_sdf_relist.
//
//   track_weno  one launch per normalisation pass, one 512-thread block per leaf of the range, thread t = the voxel
//           ((x&7)*8 + (y&7))*8 + (z&7).  The block of an unflagged leaf leaves at once.  A flagged leaf stages its own 512 values and,
//           for each of its six faces, the THREE nearest planes of the face neighbour (its planes 5, 6, 7 on the minus side, 0, 1, 2
//           on the plus side) in LDS: 512 + 6 * 3 * 64 = 1664 floats (6.5 KiB); a stencil of seven values per axis needs no edges
//           or corners.  +bg where the neighbour is unflagged or outside the range.  The 1152 halo values are staged in three
//           rounds of 512 threads, at most three per thread; the 64 threads of a wave fetch one plane, so the flag test is uniform.
//           Every thread writes its voxel to the OTHER buffer: an active voxel wdef::track_value_weno of its 19 values
//           (sdf_weno_def.h), an inactive one its value unchanged and without the arithmetic.  Jacobi by construction.
//           TRIM and ATTR: sdf_leaf.h's trim_store, as in k_sdf_track.
// Arithmetic: float and double as sdf_weno_def.h types them, no FMA (-ffp-contract=off), IEEE division and square root.
// LDS: the x axis is laid out as one column of 14 planes, T[(x + 3) * 64 + yz] for x = -3..10: the minus neighbour's planes 5, 6, 7,
// the leaf's own eight, the plus neighbour's planes 0, 1, 2.  So the voxel's own value is T[192 + t], a wave (an x plane) reads
// every x neighbour as 64 consecutive floats without a branch, and own y and z neighbours are T[192 + t +- 8 k], T[192 + t +- k].
// The y and z halos follow at T[896 + ((axis - 1) * 6 + side * 3 + d) * 64 + uv], d = 0, 1, 2 the distance from the face less one,
// uv = x*8+z for y and x*8+y for z.  Along y and z some lanes of a wave read own values and some a halo row, which can share banks;
// not measured, see DESIGN f16.
#include "common.h"
#include "sdf_leaf.h"
#include "sdf_weno_def.h"

namespace fl {

// where the tile keeps the halo value of face (axis, side) at depth d (0 = the plane that touches the leaf) and position uv
__device__ __forceinline__ int weno_halo(int axis, int side, int d, int uv)
{
    return axis == 0 ? (side ? 11 + d : 2 - d) * 64 + uv : 896 + ((axis - 1) * 6 + side * 3 + d) * 64 + uv;
}

// the value at c + k on axis 1 or 2: c = the voxel's coordinate on it, step = 8 or 1, uv = its position in the face
__device__ __forceinline__ float weno_at(const float* T, int axis, int t, int c, int k, int step, int uv)
{
    const int q = c + k;
    if (q >= 0 && q < 8) return T[192 + t + step * k];
    return q < 0 ? T[weno_halo(axis, 0, -1 - q, uv)] : T[weno_halo(axis, 1, q - 8, uv)];
}

template <bool TRIM, bool ATTR>
__global__ __launch_bounds__(512) void k_sdf_track_weno(SdfGeom g, float dt, float inv, const int* __restrict__ flags, unsigned long long* tm,
                                                        const float* src, float* dst, uint32_t* __restrict__ tid, float* __restrict__ tvel)
{
    __shared__ float T[14 * 64 + 12 * 64];
    const long j = blockIdx.x;
    if (!flags[j]) return;   // (the whole block alike)
    const int t = threadIdx.x;
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const float own = src[j * 512 + t];
    T[192 + t] = own;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int h = t + 512 * r;   // halo value h: plane h >> 6 = 3 * face + depth, position h & 63
        if (h < 18 * 64) {
            const int pl = h >> 6, uv = h & 63, f = pl / 3, d = pl - 3 * f, axis = f >> 1, side = f & 1;
            T[weno_halo(axis, side, d, uv)] = face_value(g, flags, src, j, axis, side, side ? d : 7 - d, uv);
        }
    }
    __syncthreads();
    const bool act = leaf_active(tm, j, t);
    float val = own;
    if (act) {
        const int xz = x * 8 + z, xy = t >> 3;
        float ux[7], uy[7], uz[7];
#pragma unroll
        for (int k = -3; k <= 3; ++k) {
            ux[k + 3] = T[192 + t + 64 * k];
            uy[k + 3] = weno_at(T, 1, t, y, k, 8, xz);
            uz[k + 3] = weno_at(T, 2, t, z, k, 1, xy);
        }
        val = wdef::track_value_weno(ux, uy, uz, dt, inv);
    }
    if (TRIM) val = trim_store<ATTR>(g, j, t, x, act, val, tm, tid, tvel);   // (every lane of the wave is here: the branches above have rejoined)
    dst[j * 512 + t] = val;
}

void launch_sdf_track_weno(hipStream_t st, const SdfGeom& g, bool trim, const int* flags, uint64_t* tm, const float* src, float* dst, uint32_t* tid,
                           float* tvel)
{
    const float dt = g.dxf * 0.3f, inv = 1.0f / g.dxf;
    const dim3 grid((unsigned)g.leaves()), block(512);
    unsigned long long* m = (unsigned long long*)tm;
    const bool attr = tid != nullptr;
    if (!trim) hipLaunchKernelGGL((k_sdf_track_weno<false, false>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
    else if (attr) hipLaunchKernelGGL((k_sdf_track_weno<true, true>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
    else hipLaunchKernelGGL((k_sdf_track_weno<true, false>), grid, block, 0, st, g, dt, inv, flags, m, src, dst, tid, tvel);
}

}  // namespace fl
