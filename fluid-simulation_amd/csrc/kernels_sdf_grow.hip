// The band dilation at the head of a grown track for gfx950 (wave64) (include/fluid_hip.h, "liquid surface, grown band";
// fluid_sdf.hip).  The leaves, their flags and what an unflagged leaf reads as: sdf_leaf.h.
//
//   grow    one launch per track, one 512-thread block per leaf of the range, wave x = the mask word of the (y, z) plane at x, lane =
//           the bit y * 8 + z.  Everything that decides is wave-uniform word arithmetic (sdf_grow_def.h): the in-plane neighbours are
//           shifts of the own word by 1 (with the z = 0 / z = 7 columns masked) and by 8, the x neighbours are the adjacent words,
//           and across a face the wave needs one word of the +-x leaf, a row of the same word of the +-y leaf and a bit column of
//           the same word of the +-z leaf — 7 flag loads and at most 7 word loads per wave, and no value load at all.
//           The launch READS flags and tm and WRITES flags2 and tm2, a second set the host swaps in afterwards: neighbour blocks of
//           the same launch read this leaf's flag and words, so no block may write what another reads (kernels_sdf_track.hip states
//           the same for its own launches).  Every block writes flags2[j]; the words only where flags2[j] is 1.
//           A leaf whose flag is 0 and whose new mask is not empty becomes flagged: its 512 values are set to +bg in `val`, the
//           buffer the next pass reads, and with ATTR its ids to NO_ID and its velocities to +0 — nobody reads either in this launch.
//           ATTR: a newly active voxel takes the id and velocity of its first neighbour, in the order -x +x -y +y -z +z, that was
//           active before.  tid and tvel are updated in place: only newly active voxels are written and only voxels that were
//           active are read, so the two sets are disjoint across the whole launch.
#include "common.h"
#include "sdf_grow_def.h"
#include "sdf_leaf.h"

namespace fl {

template <bool ATTR>
__global__ __launch_bounds__(512) void k_sdf_grow(SdfGeom g, const int* __restrict__ flags, const unsigned long long* __restrict__ tm,
                                                  int* __restrict__ flags2, unsigned long long* __restrict__ tm2, float* __restrict__ val,
                                                  uint32_t* tid, float* tvel)
{
    const long j = blockIdx.x;
    const int t = threadIdx.x, x = t >> 6, bit = t & 63;
    const long sx = (long)g.nl[1] * g.nl[2], sy = g.nl[2];
    int jx, jy, jz;
    leaf_coords(g, j, jx, jy, jz);
    // the six face neighbours in the range, -1 where the range ends or the leaf is not flagged: sdf_leaf.h's face_or_none rule written
    // out for all six at once, from the three coordinates (six calls of the helper cost 0.6 us a launch: profiles/track/NOTES.md)
    long nb[6];
    nb[0] = jx > 0 ? j - sx : -1, nb[1] = jx < g.nl[0] - 1 ? j + sx : -1;
    nb[2] = jy > 0 ? j - sy : -1, nb[3] = jy < g.nl[1] - 1 ? j + sy : -1;
    nb[4] = jz > 0 ? j - 1 : -1, nb[5] = jz < g.nl[2] - 1 ? j + 1 : -1;
#pragma unroll
    for (int d = 0; d < 6; ++d)
        if (nb[d] >= 0 && !flags[nb[d]]) nb[d] = -1;
    const bool flagged = flags[j] != 0;
    const long self = flagged ? j : -1;
    auto word = [&](long l, int k) -> uint64_t { return l >= 0 ? (uint64_t)tm[l * 8 + k] : 0ull; };
    const int ox = g.L0 + 8 * (g.l0[0] + jx), oy = g.L0 + 8 * (g.l0[1] + jy), oz = g.L0 + 8 * (g.l0[2] + jz);
    const uint64_t own = word(self, x);
    uint64_t c[6];
    gdef::neighbours(own, x > 0 ? word(self, x - 1) : word(nb[0], 7), x < 7 ? word(self, x + 1) : word(nb[1], 0), word(nb[2], x), word(nb[3], x),
                     word(nb[4], x), word(nb[5], x), c);
    const uint64_t fresh = (c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & gdef::grid_word(ox + x, oy, oz, g.lo, g.hi) & ~own;
    const int any = __syncthreads_or(fresh != 0);   // (every thread of the block is here)
    if (!flagged && !any) {
        if (t == 0) flags2[j] = 0;
        return;
    }
    if (t == 0) flags2[j] = 1;
    if (bit == 0) tm2[j * 8 + x] = own | fresh;
    if (!flagged) {
        val[j * 512 + t] = g.bg;
        if (ATTR) attr_clear(tid, tvel, j, t);
    }
    if (ATTR && ((fresh >> bit) & 1ull)) {
        int d = 5;   // (fresh is a subset of the union of c: some direction has the bit)
#pragma unroll
        for (int k = 4; k >= 0; --k)
            if ((c[k] >> bit) & 1ull) d = k;
        const long from = (gdef::neighbour_crosses(t, d) ? nb[d] : j);
        const int at = gdef::neighbour_offset(t, d);
        tid[j * 512 + t] = tid[from * 512 + at];
        const float* tr = tvel + from * 1536 + at;
        float* tw = tvel + j * 1536 + t;
        tw[0] = tr[0], tw[512] = tr[512], tw[1024] = tr[1024];
    }
}

void launch_sdf_grow(hipStream_t st, const SdfGeom& g, const int* flags, const uint64_t* tm, int* flags2, uint64_t* tm2, float* val, uint32_t* tid,
                     float* tvel)
{
    const dim3 grid((unsigned)g.leaves()), block(512);
    if (tid)
        hipLaunchKernelGGL((k_sdf_grow<true>), grid, block, 0, st, g, flags, (const unsigned long long*)tm, flags2, (unsigned long long*)tm2, val, tid, tvel);
    else
        hipLaunchKernelGGL((k_sdf_grow<false>), grid, block, 0, st, g, flags, (const unsigned long long*)tm, flags2, (unsigned long long*)tm2, val, tid, tvel);
}

}  // namespace fl
