// Box filter and offset of the particles' level set for gfx950 (wave64) (include/fluid_hip.h, "liquid surface, smoothed";
// fluid_sdf.hip).  The leaves, their flags and what an unflagged leaf reads as: sdf_leaf.h.
//
//   box     one launch per axis pass, one 512-thread block per leaf of the range, thread t = the voxel ((x&7)*8 + (y&7))*8 + (z&7).
//           The block of an unflagged leaf leaves at once.  A flagged leaf stages its 8 x 8 x (8 + 2W) values along the axis in LDS
//           (4 KB at W = 4): its own 512 and W planes from either neighbour leaf on that axis, +bg where that leaf is unflagged or
//           outside the range.  Every thread then writes its voxel to the OTHER buffer: an active voxel the sum of its 2W + 1
//           values in ascending order times frac, an inactive one its value unchanged.  Jacobi by construction: src is never
//           written.  The last pass of a filter adds the offset to the active voxels' results.
//   offset  the same tiling without the tile, in place: the filter with no iteration.
// Arithmetic: float, no FMA (-ffp-contract=off); frac is computed once on the host (1.0f / (float)(2W + 1), IEEE division).
// LDS index of plane k (0 .. 8 + 2W - 1) and in-plane position uv (0 .. 63): k * 64 + ((uv + 8 k) & 63).  A wave is an x plane of
// the leaf; for either in-plane numbering below its 64 lanes then fall into 64 different banks on every axis.
#include "common.h"
#include "sdf_leaf.h"

namespace fl {

__device__ __forceinline__ int box_lds(int k, int uv) { return k * 64 + ((uv + 8 * k) & 63); }

__global__ __launch_bounds__(512) void k_sdf_box(SdfGeom g, int axis, int W, float frac, float off, const int* __restrict__ flags,
                                                 const unsigned long long* __restrict__ tm, const float* __restrict__ src,
                                                 float* __restrict__ dst)
{
    __shared__ float T[64 * 16];
    const long j = blockIdx.x;
    if (!flags[j]) return;   // (the whole block alike)
    const int t = threadIdx.x;
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const int kc = axis == 0 ? x : axis == 1 ? y : z;
    const int uv = axis == 0 ? (t & 63) : axis == 1 ? x * 8 + z : t >> 3;
    const float own = src[j * 512 + t];
    T[box_lds(kc + W, uv)] = own;
    if (t < 2 * W * 64) {
        // halo plane i (0 .. W-1) of the leaf at -1 (its planes 8-W ..) or +1 (its planes 0 ..) on the axis
        const int side = t >= W * 64, r = t - side * W * 64, i = r >> 6, huv = r & 63;
        T[box_lds(side ? 8 + W + i : i, huv)] = face_value(g, flags, src, j, axis, side, side ? i : 8 - W + i, huv);
    }
    __syncthreads();
    float val = own;
    if (leaf_active(tm, j, t)) {
        float s = 0.0f;
        for (int i = 0; i <= 2 * W; ++i) s = s + T[box_lds(kc + i, uv)];
        val = s * frac;
        if (off != 0.0f) val = val + off;
    }
    dst[j * 512 + t] = val;
}

__global__ __launch_bounds__(512) void k_sdf_offset(float off, const int* __restrict__ flags, const unsigned long long* __restrict__ tm,
                                                    float* __restrict__ tv)
{
    const long j = blockIdx.x;
    if (!flags[j]) return;
    const int t = threadIdx.x;
    if (leaf_active(tm, j, t)) tv[j * 512 + t] = tv[j * 512 + t] + off;
}

void launch_sdf_box(hipStream_t st, const SdfGeom& g, int axis, int W, float off, const int* flags, const uint64_t* tm, const float* src,
                    float* dst)
{
    const float frac = 1.0f / (float)(2 * W + 1);
    hipLaunchKernelGGL(k_sdf_box, dim3((unsigned)g.leaves()), dim3(512), 0, st, g, axis, W, frac, off, flags, (const unsigned long long*)tm, src,
                       dst);
}

void launch_sdf_offset(hipStream_t st, const SdfGeom& g, float off, const int* flags, const uint64_t* tm, float* tv)
{
    hipLaunchKernelGGL(k_sdf_offset, dim3((unsigned)g.leaves()), dim3(512), 0, st, off, flags, (const unsigned long long*)tm, tv);
}

}  // namespace fl
