// The arithmetic of the velocity trails (include/fluid_hip.h, "liquid surface, velocity trails"), stated once for the kernels
// (kernels_sdf_trail.hip, hipcc) and the host functions (sdf_trail_host.cpp, g++): the step from one instance of a particle to the
// next, an instance's own constants, and what an instance says about a voxel.  Which instances a voxel meets, and in which order, is
// each side's own: an OR and a minimum of floats do not care.  Both builds state -ffp-contract=off: every product is formed before
// its sum; sqrtf and the division are IEEE.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define TDEF __host__ __device__ __forceinline__
#else
#define TDEF inline
#endif

namespace tdef {

constexpr int MAX_INSTANCES = 32;

// the limits of fluid_sdf_trails_t (Rm <= R belongs to the snapshot: radius_ok)
TDEF bool settings_ok(double shutter, double delta, double radius_min, int32_t max_instances, int32_t reserved)
{
    return shutter >= 0 && shutter <= DBL_MAX && delta > 0 && delta <= DBL_MAX && radius_min > 0 && radius_min <= DBL_MAX &&
           max_instances >= 1 && max_instances <= MAX_INSTANCES && reserved == 0;
}
TDEF bool radius_ok(double radius_min, float R) { return (float)radius_min <= R; }

// what the instances of all particles share
struct Consts {
    double shutter;
    float R, dR, c;   // dR = R - Rm, c = 0.5f * (float)delta
    int max_instances;
};
TDEF Consts consts(double shutter, double delta, double radius_min, int32_t max_instances, float R)
{
    Consts k;
    k.shutter = shutter;
    k.R = R;
    k.dR = R - (float)radius_min;
    k.c = 0.5f * (float)delta;
    k.max_instances = max_instances;
    return k;
}

// A particle's trail: instance 0 is (P0, R); next() steps to instance k + 1 and says whether there is one.  The loop is bounded by
// max_instances alone (t may stop growing in float).
struct Trail {
    float speed, inv, n[3];
    float t, r;
    int k;
    bool moving;
};
TDEF Trail trail(const Consts& c, double vx, double vy, double vz)
{
    Trail T;
    const float fx = (float)(c.shutter * vx), fy = (float)(c.shutter * vy), fz = (float)(c.shutter * vz);
    const float s2 = (fx * fx + fy * fy) + fz * fz;
    T.speed = sqrtf(s2);
    T.moving = T.speed > 0.0f && T.speed <= FLT_MAX;
    T.inv = 0.0f, T.n[0] = T.n[1] = T.n[2] = 0.0f;
    if (T.moving) {
        T.inv = 1.0f / T.speed;
        T.n[0] = -(fx * T.inv), T.n[1] = -(fy * T.inv), T.n[2] = -(fz * T.inv);
    }
    T.t = 0.0f, T.r = c.R, T.k = 0;
    return T;
}
TDEF bool next(const Consts& c, Trail& T)
{
    if (!T.moving) return false;
    T.t = T.t + c.c * T.r;
    if (!(T.t <= T.speed && T.k + 1 < c.max_instances)) return false;
    T.k = T.k + 1;
    T.r = c.R - (c.dR * T.t) * T.inv;
    return true;
}
// coordinate a of the current instance (instance 0: P0 itself, untouched)
TDEF double at(const Trail& T, double p0, int a) { return T.k == 0 ? p0 : p0 + (double)(T.t * T.n[a]); }

// An instance's own band: max2 and min2 of "liquid surface" with its radius
struct Ball {
    float r, max2, min2;
};
TDEF Ball ball(float r, float w)
{
    Ball b;
    const float mx = r + w;
    const float mn = fmaxf(0.0f, r - w);
    b.r = r, b.max2 = mx * mx, b.min2 = mn * mn;
    return b;
}

// What one instance does to a voxel's state (inside: some instance says inside; d: the minimum candidate, INFINITY: none)
TDEF void visit(bool& inside, float& d, float x2, float r, float max2, float min2, float dxf)
{
    if (x2 >= max2) return;
    if (x2 <= min2) {
        inside = true;
        return;
    }
    d = fminf(d, dxf * (sqrtf(x2) - r));
}

// the voxel from the state
TDEF void finish(bool inside, float d, float bg, float& val, bool& act)
{
    val = bg, act = false;
    if (inside) val = -bg;
    else if (d < bg) val = d, act = true;
}

// x2y2z2 of "liquid surface": differences and squares in double, one narrowing to float per axis
TDEF float dist2(int vx, int vy, int vz, double x, double y, double z)
{
    const double ax = (double)vx - x, ay = (double)vy - y, az = (double)vz - z;
    const float x2 = (float)(ax * ax);
    const float x2y2 = (float)((double)x2 + ay * ay);
    return (float)((double)x2y2 + az * az);
}

}  // namespace tdef
