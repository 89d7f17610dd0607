// What every level-set pass does with a leaf and its neighbours, stated once for kernels_sdf_{filter,track,weno,grow,flow}.hip
// (device code only; the schedule is sdf_filter_plan.h's and the per-voxel arithmetic sdf_*_def.h's).
// The passes work on what k_sdf_search (kernels_sdf.hip) leaves on the device: tv (512 values), tm (8 mask words) and a flag per
// leaf j = (jx * nl[1] + jy) * nl[2] + jz of the range, a dense box of leaves, so that a neighbour's index is arithmetic.  Voxel
// t = ((x&7)*8 + (y&7))*8 + (z&7) of a leaf is bit t & 63 of its mask word t >> 6: a wave of a 512-thread block is an x plane.
// A leaf whose flag is 0 is inactive +bg everywhere WHATEVER its tv and tm hold (they may be those of an earlier snapshot), and so
// is every leaf outside the range and everything outside the grid: only flagged leaves are ever read, and only flagged leaves are
// written.  The flag means "this leaf's values are valid": no pass clears it, because the neighbour blocks of the same launch read
// it to choose between src and +bg.  A flagged leaf that a trim left all inactive +bg reads correctly; whether a leaf is LISTED is
// derived afterwards (k_sdf_relist), into an array of its own.
#pragma once
#include "common.h"
#include "sdf_track_def.h"

namespace fl {

// offset in the leaf of the voxel at plane k of the axis and in-plane position uv: uv = y*8+z (axis x), x*8+z (y), x*8+y (z)
__device__ __forceinline__ int leaf_voxel(int axis, int k, int uv)
{
    return axis == 0 ? k * 64 + uv : axis == 1 ? (uv >> 3) * 64 + k * 8 + (uv & 7) : uv * 8 + k;
}

// leaf j of the range as (jx, jy, jz)
__device__ __forceinline__ void leaf_coords(const SdfGeom& g, long j, int& jx, int& jy, int& jz)
{
    jz = (int)(j % g.nl[2]), jy = (int)((j / g.nl[2]) % g.nl[1]), jx = (int)(j / ((long)g.nl[1] * g.nl[2]));
}

// is voxel t of leaf j active?
__device__ __forceinline__ bool leaf_active(const unsigned long long* __restrict__ tm, long j, int t)
{
    return (tm[j * 8 + (t >> 6)] >> (t & 63)) & 1ull;
}

// A neighbour leaf reads as +bg unless it is inside the range AND flagged.  That rule in its two shapes: found(q) is called with the
// leaf's index if it is there, and nothing happens if not.  (A body passed in, and not an index-or-minus-one handed back: the
// callers' "else +bg" then compiles to the nested branch it was; a sentinel compiled to selects and, in k_sdf_box, to a flat load.)
// Leaf (qx, qy, qz), any of the 26 around a leaf ...
template <typename Found>
__device__ __forceinline__ void leaf_or_none(const SdfGeom& g, const int* __restrict__ flags, int qx, int qy, int qz, Found found)
{
    if (qx >= 0 && qx < g.nl[0] && qy >= 0 && qy < g.nl[1] && qz >= 0 && qz < g.nl[2]) {
        const long q = ((long)qx * g.nl[1] + qy) * g.nl[2] + qz;
        if (flags[q]) found(q);
    }
}
// ... and the face neighbour of leaf j on (axis, side), side 0 = -1, 1 = +1: one coordinate moves, so one range test and j -+ a stride
template <typename Found>
__device__ __forceinline__ void face_or_none(const SdfGeom& g, const int* __restrict__ flags, long j, int axis, int side, Found found)
{
    const int ja = axis == 0 ? (int)(j / ((long)g.nl[1] * g.nl[2])) : axis == 1 ? (int)((j / g.nl[2]) % g.nl[1]) : (int)(j % g.nl[2]);
    const long stride = axis == 0 ? (long)g.nl[1] * g.nl[2] : axis == 1 ? g.nl[2] : 1;
    const int jn = ja + (side ? 1 : -1);
    if (jn >= 0 && jn < g.nl[axis]) {
        const long q = side ? j + stride : j - stride;
        if (flags[q]) found(q);
    }
}

// the value at `plane` of the axis and in-plane position uv in the face neighbour of leaf j on (axis, side), +bg where there is none
__device__ __forceinline__ float face_value(const SdfGeom& g, const int* __restrict__ flags, const float* src, long j, int axis, int side,
                                            int plane, int uv)
{
    float v = g.bg;
    face_or_none(g, flags, j, axis, side, [&](long q) { v = src[q * 512 + leaf_voxel(axis, plane, uv)]; });
    return v;
}

// voxel t of leaf j carries no particle: NO_ID and +0
__device__ __forceinline__ void attr_clear(uint32_t* __restrict__ tid, float* __restrict__ tvel, long j, int t)
{
    tid[j * 512 + t] = 0xffffffffu;
    float* tw = tvel + j * 1536 + t;
    tw[0] = 0.0f, tw[512] = 0.0f, tw[1024] = 0.0f;
}

// TRIM (the last pass of a track), for voxel t of leaf j in wave x, active or not with the result val: an active result at or
// beyond +-bg becomes inactive +-bg, and with ATTR its id and velocity NO_ID and +0; the wave's ballot of "still active" is the new
// mask word x, written over tm[j*8 + x] — only this wave reads that word.  Returns the value to store.
template <bool ATTR>
__device__ __forceinline__ float trim_store(const SdfGeom& g, long j, int t, int x, bool act, float val, unsigned long long* tm,
                                            uint32_t* __restrict__ tid, float* __restrict__ tvel)
{
    const int cls = act ? tdef::trim_class(val, g.bg) : 0;
    if (cls != 0) {
        val = cls < 0 ? -g.bg : g.bg;
        act = false;
        if (ATTR) attr_clear(tid, tvel, j, t);
    }
    const unsigned long long b = __ballot(act);   // (every lane of the wave is here: the branches above have rejoined)
    if ((t & 63) == 0) tm[j * 8 + x] = b;
    return val;
}

}  // namespace fl
