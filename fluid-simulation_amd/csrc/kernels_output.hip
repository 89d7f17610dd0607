// Leaf compaction of the output grid for gfx950 (wave64, 256-thread blocks): which of OpenVDB's 8^3 leaves of the density
// grid hold anything but +0, and those leaves packed as 2 KB records in the leaf's own voxel order (fluid_output.hip).
//
// Leaves have their origins at multiples of 8 in index space.  Array index a of an axis holds coordinate lo + a, the first
// leaf starts at L0 = lo & ~7, so leaf l of an axis covers the array indices off + 8 l .. off + 8 l + 7 with off = L0 - lo
// in (-8, 0] (N = 121: off = -4, the first leaf holds 4 in-grid cells per axis; N = 256: off = 0).
// A leaf is listed iff an in-grid voxel of it has a non-zero BIT PATTERN (-0.0f and NaN count).  No atomics, no
// floating-point arithmetic: the list and the records are a function of the field alone.
#include "common.h"

namespace fl {

// The array is a window (nx, ny, nz) of the grid whose cell 0 is global array index (ox, oy, oz); the handle owns the global
// indices [olo, ohi) per axis, inside the window (OutWin).  On one GPU window = grid = owned block: origin 0, dims N, [0, N).
// On a rank of a decomposed run everything else the array holds (halo cells; in replicated mode the rest of the full-size array)
// is other ranks' sums or partial sums: it neither lists a leaf nor reaches a record.  The leaves looked at are the GLOBAL leaves
// that meet the owned block, l0 .. l0 + nl - 1 per axis; local number = ((lx - l0x) nly + (ly - l0y)) nlz + (lz - l0z), ascending
// with the (x, y, z) origin.

// One block per (leaf-x, leaf-y) column of the leaf range: its 64 (x, y) rows are streamed along z, lanes on consecutive z.  A
// wave ORs the bit patterns of its 16 rows in registers, one ballot per 64-cell stretch of z gives 8 leaves' flags (one byte
// each), the four waves meet in LDS.  Reads every owned float of the container once; rows of an odd N or of a window are not
// 16-byte aligned: dword loads, 16 of them in flight per lane (every load is issued before the first is needed; a voxel outside
// the owned block reads cell 0 and is masked).
__global__ __launch_bounds__(256) void k_out_mark(const float* __restrict__ f, OutWin w, int* __restrict__ flags)
{
    __shared__ int hit[4][136];   // nl[2] <= 129 (N <= 1024; checked by the host)
    const int jx = blockIdx.x / w.nl[1], jy = blockIdx.x % w.nl[1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t* __restrict__ u = (const uint32_t*)f;
    const int gx0 = w.off + 8 * (w.l0[0] + jx), gy0 = w.off + 8 * (w.l0[1] + jy), gz0 = w.off + 8 * w.l0[2];
    for (int k = 0; k * 8 < w.nl[2]; ++k) {
        const int gz = gz0 + 64 * k + lane;
        const bool zin = gz >= w.olo[2] && gz < w.ohi[2];
        uint32_t v[16], inm = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = wv + 4 * i;
            const int gx = gx0 + (r >> 3), gy = gy0 + (r & 7);
            const bool in = zin && gx >= w.olo[0] && gx < w.ohi[0] && gy >= w.olo[1] && gy < w.ohi[1];
            v[i] = u[in ? ((size_t)(gx - w.ox) * w.ny + (gy - w.oy)) * w.nz + (gz - w.oz) : 0];
            inm |= (in ? 1u : 0u) << i;
        }
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc |= ((inm >> i) & 1u) ? v[i] : 0u;
        const unsigned long long b = __ballot(acc != 0);
        if (lane < 8 && 8 * k + lane < w.nl[2]) hit[wv][8 * k + lane] = ((b >> (8 * lane)) & 0xffull) != 0;
    }
    __syncthreads();
    for (int jz = threadIdx.x; jz < w.nl[2]; jz += 256)
        flags[((size_t)jx * w.nl[1] + jy) * w.nl[2] + jz] = hit[0][jz] | hit[1][jz] | hit[2][jz] | hit[3][jz];
}

// One wave per leaf of the range; the waves of unlisted leaves leave at once.  Lane = (x, y) row of the leaf: its 8 z values are
// the lane's 32 contiguous bytes of the record, values[((x&7)*8 + (y&7))*8 + (z&7)]; a voxel the handle does not own (halo, another
// rank's, outside the grid) holds +0.  slot[leaf] is the exclusive scan of the flags: the record's place in the list.
__global__ __launch_bounds__(256) void k_out_pack(const float* __restrict__ f, OutWin w, long nleaf, const int* __restrict__ flags,
                                                  const int* __restrict__ slot, float* __restrict__ values, int* __restrict__ origin)
{
    const long leaf = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (leaf >= nleaf || !flags[leaf]) return;
    const int lane = threadIdx.x & 63;
    const int lz = w.l0[2] + (int)(leaf % w.nl[2]), ly = w.l0[1] + (int)((leaf / w.nl[2]) % w.nl[1]), lx = w.l0[0] + (int)(leaf / ((long)w.nl[1] * w.nl[2]));
    const long s = slot[leaf];
    const int gx = w.off + 8 * lx + (lane >> 3), gy = w.off + 8 * ly + (lane & 7), gz0 = w.off + 8 * lz;
    const bool rin = gx >= w.olo[0] && gx < w.ohi[0] && gy >= w.olo[1] && gy < w.ohi[1];
    float v[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) {
        const int gz = gz0 + z;
        v[z] = (rin && gz >= w.olo[2] && gz < w.ohi[2]) ? f[((size_t)(gx - w.ox) * w.ny + (gy - w.oy)) * w.nz + (gz - w.oz)] : 0.0f;
    }
    float4* dst = (float4*)(values + s * 512 + lane * 8);   // 32-byte aligned: the record base is hipMalloc's
    dst[0] = make_float4(v[0], v[1], v[2], v[3]);
    dst[1] = make_float4(v[4], v[5], v[6], v[7]);
    if (lane < 3) origin[s * 3 + lane] = w.lo + w.off + 8 * (lane == 0 ? lx : lane == 1 ? ly : lz);
}

void launch_out_mark(hipStream_t st, const float* f, const OutWin& w, int* flags)
{
    hipLaunchKernelGGL(k_out_mark, dim3((unsigned)(w.nl[0] * w.nl[1])), dim3(256), 0, st, f, w, flags);
}

void launch_out_pack(hipStream_t st, const float* f, const OutWin& w, const int* flags, const int* slot, float* values, int* origin)
{
    const long nleaf = w.leaves();
    hipLaunchKernelGGL(k_out_pack, dim3((unsigned)((nleaf + 3) / 4)), dim3(256), 0, st, f, w, nleaf, flags, slot, values, origin);
}

}  // namespace fl
