// The per-voxel arithmetic of the HJWENO5 renormalisation (include/fluid_hip.h, "liquid surface, renormalised: HJWENO5"), stated
// once for the kernel (kernels_sdf_weno.hip, hipcc) and the host function (sdf_filter_host.cpp, g++): the fifth-order WENO
// interpolation of five one-sided differences, the two biased differences of an axis from its seven values, and one pass on an
// active voxel from its 19 values.  Only the gradient term differs from sdf_track_def.h: the Godunov selection (tdef::axis_term)
// and the step (tdef::track_step, the tail of tdef::track_value) are that file's.  How the 18 neighbours are fetched, who is active
// and where things are written is each side's own.  Both builds state -ffp-contract=off: every product is formed before its sum,
// in float and in double.  Restated from OpenVDB's math/FiniteDifference.h:331-349 (WENO5), 1224-1233 and 1428-1435 (D1<FD_HJWENO5>,
// D1<BD_HJWENO5>), 352-374 (GodunovsNormSqrd), math/Operators.h:252-284 and tools/LevelSetTracker.h:596-609.
#pragma once
#include "sdf_track_def.h"

namespace wdef {

TDEF float sqf(float a) { return a * a; }
TDEF double sqd(double a) { return a * a; }

// WENO5<float>(v1..v5, scale2 = 0.01f): float where the library's expression is float, double where it promotes
TDEF float weno5(float v1, float v2, float v3, float v4, float v5)
{
    const double C = 13.0 / 12.0;
    const double eps = 1.0e-6 * (double)0.01f;
    const double s1 = (C * (double)sqf((v1 - 2.0f * v2) + v3) + 0.25 * sqd((double)(v1 - 4.0f * v2) + 3.0 * (double)v3)) + eps;
    const double s2 = (C * (double)sqf((v2 - 2.0f * v3) + v4) + 0.25 * (double)sqf(v2 - v4)) + eps;
    const double s3 = (C * (double)sqf((v3 - 2.0f * v4) + v5) + 0.25 * sqd((3.0 * (double)v3 - (double)(4.0f * v4)) + (double)v5)) + eps;
    const double A1 = 0.1 / (s1 * s1), A2 = 0.6 / (s2 * s2), A3 = 0.3 / (s3 * s3);
    const double d1 = v1, d2 = v2, d3 = v3, d4 = v4, d5 = v5;
    const double num = (A1 * ((2.0 * d1 - 7.0 * d2) + 11.0 * d3) + A2 * ((5.0 * d3 - d2) + 2.0 * d4)) + A3 * ((2.0 * d3 + 5.0 * d4) - d5);
    return (float)((double)(float)num / (6.0 * ((A1 + A2) + A3)));
}

// The biased differences of one axis: u[k + 3] = val(c + k e_a), k = -3..3.  dm looks down (BD_HJWENO5), dp up (FD_HJWENO5).
TDEF void axis_diffs(const float u[7], float& dm, float& dp)
{
    dp = weno5(u[6] - u[5], u[5] - u[4], u[4] - u[3], u[3] - u[2], u[2] - u[1]);
    dm = -weno5(u[0] - u[1], u[1] - u[2], u[2] - u[3], u[3] - u[4], u[4] - u[5]);
}

// One pass on an active voxel: x, y, z hold the axis' seven values, the voxel's own value p in the middle of each.
TDEF float track_value_weno(const float x[7], const float y[7], const float z[7], float dt, float inv)
{
    const float p = x[3];
    const bool out = p > 0.0f;
    float dm, dp;
    axis_diffs(x, dm, dp);
    const float tx = tdef::axis_term(out, dm, dp);
    axis_diffs(y, dm, dp);
    const float ty = tdef::axis_term(out, dm, dp);
    axis_diffs(z, dm, dp);
    const float tz = tdef::axis_term(out, dm, dp);
    return tdef::track_step(p, tx, ty, tz, dt, inv);
}

}  // namespace wdef
