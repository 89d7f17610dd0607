// The per-voxel arithmetic of the averaged-position surface (include/fluid_hip.h, "liquid surface, averaged positions"), stated
// once for the kernel (kernels_sdf_avg.hip, hipcc) and the host function (sdf_avg_host.cpp, g++): the squared distance of "liquid
// surface", a particle's integer weight and offset, and the finish from the minimum and the four integer sums to the voxel's value
// and state.  Which particles a voxel meets, and in which order, is each side's own: a minimum and wrapping integer sums do not
// care.  Both builds state -ffp-contract=off: every product is formed before its sum; sqrtf and the divisions are IEEE.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define ADEF __host__ __device__ __forceinline__
#else
#define ADEF inline
#endif

namespace adef {

constexpr float W_ONE = 16777216.0f;    // 2^24: a weight of 1
constexpr double O_ONE = 262144.0;      // 2^18: an offset of one voxel
constexpr int LAST_RING = 4;            // hf <= 4 and R + w <= 4: no particle further out than ring 4 weighs or lowers a value in the band

struct Consts {
    float h2, ih2;   // hf * hf and 1.0f / h2, both rounded to float
};

ADEF bool influence_ok(double influence)
{
    const float hf = (float)influence;
    return influence > 0 && hf > 0.0f && hf <= 4.0f;
}

ADEF Consts consts(double influence)
{
    const float hf = (float)influence;
    Consts c;
    c.h2 = hf * hf;
    c.ih2 = 1.0f / c.h2;
    return c;
}

// The last ring of cells a voxel has to see: a particle in ring k + 1 has x2 >= (k + 0.5)^2 as computed, so neither weighs
// ((k + 0.5)^2 >= h2) nor lies inside the band ((k + 0.5)^2 >= max2) once both hold.
ADEF int last_ring(float h2, float max2)
{
    const float reach = h2 > max2 ? h2 : max2;
    int k = 0;
    while (k < LAST_RING && !(((float)k + 0.5f) * ((float)k + 0.5f) >= reach)) ++k;
    return k;
}

// x2y2z2 of "liquid surface": differences and squares in double, one narrowing to float per axis
ADEF float dist2(int vx, int vy, int vz, double x, double y, double z)
{
    const double ax = (double)vx - x, ay = (double)vy - y, az = (double)vz - z;
    const float x2 = (float)(ax * ax);
    const float x2y2 = (float)((double)x2 + ay * ay);
    return (float)((double)x2y2 + az * az);
}

// the same from the x term alone (one wave of the kernel shares it)
ADEF float dist2_x(double ax) { return (float)(ax * ax); }
ADEF float dist2_yz(float x2, int vy, int vz, double y, double z)
{
    const double ay = (double)vy - y, az = (double)vz - z;
    const float x2y2 = (float)((double)x2 + ay * ay);
    return (float)((double)x2y2 + az * az);
}

// W of a particle at squared distance x2 < h2 (the caller has asked): 0 .. 2^24, half to even
ADEF int32_t weight(float x2, Consts c)
{
    const float t = 1.0f - x2 * c.ih2;
    const float wt = (t * t) * t;
    return (int32_t)rintf(wt * W_ONE);
}

// O_a of a particle coordinate p and a voxel coordinate v; |O_a| < 2^20 wherever the weight is not 0, and < 2^21 inside ring 4
ADEF int32_t offset(double p, int v) { return (int32_t)rint((p - (double)v) * O_ONE); }

// what one particle adds to the sums, which wrap (unsigned): W * O_a is exact in 64 bits
struct Sums {
    uint64_t w = 0, x = 0, y = 0, z = 0;
};
ADEF void add(Sums& s, int32_t W, int32_t ox, int32_t oy, int32_t oz)
{
    s.w += (uint64_t)(int64_t)W;
    s.x += (uint64_t)((int64_t)W * (int64_t)ox);
    s.y += (uint64_t)((int64_t)W * (int64_t)oy);
    s.z += (uint64_t)((int64_t)W * (int64_t)oz);
}

// da of a voxel whose SW > 0
ADEF float averaged_distance(const Sums& s, float dxf, float R)
{
    const double den = (double)(int64_t)s.w * O_ONE;
    const double ax = (double)(int64_t)s.x / den, ay = (double)(int64_t)s.y / den, az = (double)(int64_t)s.z / den;
    float a2 = (float)(ax * ax);
    a2 = (float)((double)a2 + ay * ay);
    a2 = (float)((double)a2 + az * az);
    return dxf * (sqrtf(a2) - R);
}

// The voxel from m (INFINITY: no particle) and the sums.  averaged == false: "liquid surface" itself, the sums are not read.
ADEF void finish(float m, const Sums& s, bool averaged, float R, float dxf, float bg, float max2, float min2, float& val, bool& act)
{
    val = bg, act = false;
    if (!(m < max2)) return;
    if (m <= min2) {
        val = -bg;
        return;
    }
    float d = dxf * (sqrtf(m) - R);
    if (averaged && (int64_t)s.w > 0) d = fmaxf(averaged_distance(s, dxf, R), d);
    if (d < bg) val = d, act = true;
}

}  // namespace adef
