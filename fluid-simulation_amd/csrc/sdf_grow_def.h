// The mask-word arithmetic of the band dilation (include/fluid_hip.h, "liquid surface, grown band"), stated once for the kernel
// (kernels_sdf_grow.hip, hipcc) and the host function (sdf_filter_host.cpp, g++).  A leaf's mask is 8 words; word x is the (y, z)
// plane at x, voxel (y, z) at bit y * 8 + z (OpenVDB's NodeMask order).  Who the neighbour leaves are, whether they count, and
// where the result goes is each side's own.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define GDEF __host__ __device__ __forceinline__
#else
#define GDEF inline
#endif

namespace gdef {

constexpr uint64_t COL0 = 0x0101010101010101ull;   // the bits with z = 0
constexpr uint64_t COL7 = 0x8080808080808080ull;   // the bits with z = 7

// The in-grid bits of plane cx of the leaf whose y, z origin is (oy, oz); the grid is [lo,hi]^3.
GDEF uint64_t grid_word(int cx, int oy, int oz, int lo, int hi)
{
    if (cx < lo || cx > hi) return 0;
    uint64_t row = 0, w = 0;
    for (int z = 0; z < 8; ++z)
        if (oz + z >= lo && oz + z <= hi) row |= 1ull << z;
    for (int y = 0; y < 8; ++y)
        if (oy + y >= lo && oy + y <= hi) w |= row << (8 * y);
    return w;
}

// c[d], d = -x +x -y +y -z +z: the voxels of a plane whose neighbour in direction d is active.  own = the plane's word; xm, xp =
// the words of the planes at x - 1 and x + 1 (the own leaf's, or word 7 / word 0 of the leaf across the face); ym, yp, zm, zp =
// the SAME plane's word of the leaf at -y, +y, -z, +z.  A word of a leaf that does not count is passed as 0.
GDEF void neighbours(uint64_t own, uint64_t xm, uint64_t xp, uint64_t ym, uint64_t yp, uint64_t zm, uint64_t zp, uint64_t c[6])
{
    c[0] = xm;
    c[1] = xp;
    c[2] = (own << 8) | (ym >> 56);
    c[3] = (own >> 8) | (yp << 56);
    c[4] = ((own << 1) & ~COL0) | ((zm >> 7) & COL0);
    c[5] = ((own >> 1) & ~COL7) | ((zp << 7) & COL7);
}

// offset in its leaf of the neighbour in direction d of the voxel at offset `at`, the leaf's faces wrapped: x -+ 1 is at -+ 64
GDEF int neighbour_offset(int at, int d)
{
    const int axis = d >> 1, shift = axis == 0 ? 6 : axis == 1 ? 3 : 0;
    const int k = ((at >> shift) & 7) + ((d & 1) ? 1 : -1);
    return (at & ~(7 << shift)) | ((k & 7) << shift);
}
// does that neighbour lie in the leaf across the face?
GDEF bool neighbour_crosses(int at, int d)
{
    const int axis = d >> 1, shift = axis == 0 ? 6 : axis == 1 ? 3 : 0;
    const int k = (at >> shift) & 7;
    return (d & 1) ? k == 7 : k == 0;
}

}  // namespace gdef
