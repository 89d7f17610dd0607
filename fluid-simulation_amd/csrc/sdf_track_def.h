// The per-voxel arithmetic of the renormalisation (include/fluid_hip.h, "liquid surface, renormalised"), stated once for the
// kernel (kernels_sdf_track.hip, hipcc) and the host function (sdf_filter_host.cpp, g++): one first-order upwind (Godunov) step of
// the re-initialisation equation on an active voxel, the trim class of a value, and the steps an offset is taken in.  How the six
// neighbours are fetched, who is active and where things are written is each side's own.  Both builds state -ffp-contract=off:
// every product is formed before its sum.  Restated from OpenVDB's tools/LevelSetTracker.h:293-306, 455-475, 485-494, 596-609,
// math/Operators.h:252-284, math/FiniteDifference.h:352-374, math/Math.h:118 and tools/LevelSetFilter.h:352-368.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define TDEF __host__ __device__ __forceinline__
#else
#define TDEF inline
#endif

namespace tdef {

constexpr int MAX_PASSES = 8;     // normalisation passes per track: 0..8
constexpr float TOL = 1e-8f;      // math::Tolerance<float>

// std::max / std::min: the first argument unless the second is strictly beyond it
TDEF float fmax2(float a, float b) { return a < b ? b : a; }
TDEF float fmin2(float a, float b) { return b < a ? b : a; }

// Godunov's squared one-sided difference along one axis: dm = p - val(c - e), dp = val(c + e) - p
TDEF float axis_term(bool out, float dm, float dp)
{
    const float A = out ? fmax2(dm, 0.0f) : fmin2(dm, 0.0f);
    const float B = out ? fmin2(dp, 0.0f) : fmax2(dp, 0.0f);
    return fmax2(A * A, B * B);
}

// The step from the three axis terms, whatever scheme formed them (sdf_weno_def.h forms them from seven values per axis)
TDEF float track_step(float p, float tx, float ty, float tz, float dt, float inv)
{
    float G = tx;
    G = G + ty;
    G = G + tz;
    const float S = p / (sqrtf(p * p + G) + TOL);
    return p - (dt * S) * (sqrtf(G) * inv - 1.0f);
}

// One pass on an active voxel with value p and the six neighbours' values of the pass before; dt = dx * 0.3f, inv = 1.0f / dx.
TDEF float track_value(float p, float xm, float xp, float ym, float yp, float zm, float zp, float dt, float inv)
{
    const bool out = p > 0.0f;
    const float tx = axis_term(out, p - xm, xp - p);
    const float ty = axis_term(out, p - ym, yp - p);
    const float tz = axis_term(out, p - zm, zp - p);
    return track_step(p, tx, ty, tz, dt, inv);
}

// The trim class of an active voxel's value: -1 = it becomes inactive -bg, +1 = inactive +bg, 0 = it stays as it is
TDEF int trim_class(float v, float bg) { return v <= -bg ? -1 : v >= bg ? 1 : 0; }

// The steps of a tracked offset: a = fabsf(off), d = what has been taken so far.  Returns the next step's size, 0.0f when done.
TDEF float offset_step(float a, float d, float dx)
{
    const float CFL = 0.5f * dx;
    const float rest = a - d;
    if (!(rest > 0.001f * CFL)) return 0.0f;
    return rest < CFL ? rest : CFL;
}

}  // namespace tdef
