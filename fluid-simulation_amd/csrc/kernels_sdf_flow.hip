// Median, Laplacian and mean-curvature flow of the particles' level set for gfx950 (wave64) (include/fluid_hip.h, "liquid surface,
// flows"; fluid_sdf.hip).  The kernel works on what k_sdf_search, the box passes and the tracks leave on the device; the leaves, their
// flags and what an unflagged leaf reads as: sdf_leaf.h.
//
//   flow    one launch per pass, one 512-thread block per leaf of the range, thread t = the voxel ((x&7)*8 + (y&7))*8 + (z&7).  The
//           block of an unflagged leaf leaves at once.  A flagged leaf stages its (8 + 2H)^3 tile in LDS, H = 1 (Laplacian,
//           curvature, median of width 1) or 2 (median of width 2): its own 512 values and the halo from up to 26 neighbour
//           leaves, +bg where a leaf is unflagged or outside the range.  The range is a dense box of leaves, so a neighbour's index
//           is arithmetic.  Every thread then writes its voxel to the OTHER buffer: an active voxel the value of sdf_flow_def.h for
//           the kind, an inactive one its value unchanged.  Jacobi by construction: src is never written.  The last pass of an
//           untracked filter adds the offset to the active voxels' results.
//           The Laplacian reads 7 and the curvature 19 points of the tile (no corners); both stage the whole H = 1 tile, one loader.
//           The median's tile holds the monotone KEYS of the values, and the selection (fdef::median_select: 32 sweeps over the
//           27 or 125 keys, read from the tile and not stored by the source; the compiler hoists the reads out of the sweeps and
//           keeps the keys in registers, 132 VGPRs at W = 2 and no scratch) returns the key of the median.
// Arithmetic: float and, for the curvature term, double; no FMA (-ffp-contract=off), IEEE division and square root.
// LDS: voxel (X, Y, Z) of the tile, 0 <= X, Y, Z < S = 8 + 2H, at (X * S + Y) * 24 + Z: 9.4 KB (H = 1) or 13.5 KB (H = 2), so that
// four blocks fit a CU many times over.  The row pitch is 24 words, not S, for the reads: a wave is an x plane of the leaf, a
// ds_read_b32 is served in two groups of 32 lanes = 4 rows y of 8 lanes z each, and the 4 rows start 24 words apart, at banks
// 0, 24, 16, 8 (mod 32) of wherever the stencil's offset puts them: 32 different banks for every offset.  With pitch S (10 or 12) the
// fourth row would share 6 or 8 banks with the first.  The staging loop's stores run along z and break at row ends: two-way
// conflicts at most, which a ds_write_b32 absorbs; it runs once per pass.
#include "../../include/fluid_hip.h"
#include "common.h"
#include "sdf_flow_def.h"
#include "sdf_leaf.h"

namespace fl {

constexpr int FLOW_PITCH = 24;

template <int KIND, int H>
__global__ __launch_bounds__(512) void k_sdf_flow(SdfGeom g, float invdx2, float dt, float off, const int* __restrict__ flags,
                                                  const unsigned long long* __restrict__ tm, const float* __restrict__ src,
                                                  float* __restrict__ dst)
{
    constexpr int S = 8 + 2 * H, P = FLOW_PITCH;
    constexpr bool MEDIAN = KIND == FLUID_SDF_FILTER_MEDIAN;
    __shared__ uint32_t T[S * S * P];   // the values' bits, or for the median their keys
    const long j = blockIdx.x;
    if (!flags[j]) return;   // (the whole block alike)
    const int t = threadIdx.x;
    int jx, jy, jz;
    leaf_coords(g, j, jx, jy, jz);
    const uint32_t bg = __float_as_uint(g.bg);
    for (int i = t; i < S * S * S; i += 512) {
        const int X = i / (S * S), Y = (i / S) % S, Z = i % S;
        const int rx = X - H, ry = Y - H, rz = Z - H;   // the voxel in this leaf's frame: -H .. 7 + H
        const int sx = rx < 0 ? -1 : rx >= 8 ? 1 : 0, sy = ry < 0 ? -1 : ry >= 8 ? 1 : 0, sz = rz < 0 ? -1 : rz >= 8 ? 1 : 0;
        uint32_t v = bg;
        leaf_or_none(g, flags, jx + sx, jy + sy, jz + sz,
                     [&](long q) { v = __float_as_uint(src[q * 512 + ((rx - 8 * sx) * 8 + (ry - 8 * sy)) * 8 + (rz - 8 * sz)]); });
        T[(X * S + Y) * P + Z] = MEDIAN ? fdef::median_key(v) : v;
    }
    __syncthreads();
    const int x = t >> 6, y = (t >> 3) & 7, z = t & 7;
    const int c = ((x + H) * S + (y + H)) * P + (z + H);
    const float own = src[j * 512 + t];
    float val = own;
    if (leaf_active(tm, j, t)) {
        auto at = [&](int a, int b, int d) { return __uint_as_float(T[c + (a * S + b) * P + d]); };
        if (MEDIAN) {
            constexpr int n = 2 * H + 1, m = n * n * n;
            val = __uint_as_float(fdef::median_bits(
                fdef::median_select(m, (m - 1) >> 1, [&](int i) { return T[c + ((i / (n * n) - H) * S + (i / n % n - H)) * P + (i % n - H)]; })));
        } else if (KIND == FLUID_SDF_FILTER_LAPLACIAN) {
            val = fdef::laplacian_value(own, at(-1, 0, 0), at(1, 0, 0), at(0, -1, 0), at(0, 1, 0), at(0, 0, -1), at(0, 0, 1), invdx2, dt);
        } else {
            const fdef::Edges e{at(1, 1, 0), at(1, -1, 0), at(-1, -1, 0), at(-1, 1, 0), at(1, 0, 1), at(1, 0, -1), at(-1, 0, -1), at(-1, 0, 1),
                                at(0, 1, 1), at(0, 1, -1), at(0, -1, -1), at(0, -1, 1)};
            val = fdef::curvature_value(own, at(-1, 0, 0), at(1, 0, 0), at(0, -1, 0), at(0, 1, 0), at(0, 0, -1), at(0, 0, 1), e, invdx2, dt);
        }
        if (off != 0.0f) val = val + off;
    }
    dst[j * 512 + t] = val;
}

void launch_sdf_flow(hipStream_t st, const SdfGeom& g, int kind, int W, float off, const int* flags, const uint64_t* tm, const float* src,
                     float* dst)
{
    const fdef::Consts k = fdef::consts(g.dxf);
    const dim3 grid((unsigned)g.leaves()), block(512);
    const unsigned long long* m = (const unsigned long long*)tm;
    if (kind == FLUID_SDF_FILTER_MEDIAN && W == 1)
        hipLaunchKernelGGL((k_sdf_flow<FLUID_SDF_FILTER_MEDIAN, 1>), grid, block, 0, st, g, 0.0f, 0.0f, off, flags, m, src, dst);
    else if (kind == FLUID_SDF_FILTER_MEDIAN)
        hipLaunchKernelGGL((k_sdf_flow<FLUID_SDF_FILTER_MEDIAN, 2>), grid, block, 0, st, g, 0.0f, 0.0f, off, flags, m, src, dst);
    else if (kind == FLUID_SDF_FILTER_LAPLACIAN)
        hipLaunchKernelGGL((k_sdf_flow<FLUID_SDF_FILTER_LAPLACIAN, 1>), grid, block, 0, st, g, k.invdx2, k.dt_lap, off, flags, m, src, dst);
    else
        hipLaunchKernelGGL((k_sdf_flow<FLUID_SDF_FILTER_MEAN_CURVATURE, 1>), grid, block, 0, st, g, k.invdx2, k.dt_curv, off, flags, m, src, dst);
}

}  // namespace fl
