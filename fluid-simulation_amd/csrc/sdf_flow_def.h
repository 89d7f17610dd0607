// The per-voxel arithmetic of the level-set flows (include/fluid_hip.h, "liquid surface, flows"), stated once for the kernels
// (kernels_sdf_flow.hip, hipcc) and the host function (sdf_filter_host.cpp, g++): the Laplacian step, the mean-curvature step and
// the median's selection.  How the neighbours are fetched, who is active and where things are written is each side's own.  Both
// builds state -ffp-contract=off: every product is formed before its sum.  Restated from OpenVDB's tools/LevelSetFilter.h:380-409,
// 421-450, 481-507 and math/Stencils.h:147-155, 1230-1238, 1283-1288, 1506-1540, 1596-1619, 1670-1680; math/Math.h:119.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define FDEF __host__ __device__ __forceinline__
#else
#define FDEF inline
#endif

namespace fdef {

// the constants of a flow, formed once on the host from dx = (float)params.dx (a kernel takes them as arguments)
struct Consts {
    float invdx2;    // (float)(4.0 * inv2dx * inv2dx), inv2dx = (float)(0.5 / dx): the stencils' mInvDx2
    float dt_lap;    // (dx * dx) / 6.0f
    float dt_curv;   // (dx * dx) / 3.0f
};
inline Consts consts(float dx)
{
    const float inv2dx = (float)(0.5 / (double)dx);
    return {(float)(4.0 * (double)inv2dx * (double)inv2dx), (dx * dx) / 6.0f, (dx * dx) / 3.0f};
}

// GradStencil::laplacian and the explicit step: the six face neighbours summed in the order -x +x -y +y -z +z
FDEF float laplacian_value(float p, float xm, float xp, float ym, float yp, float zm, float zp, float invdx2, float dt)
{
    float s = xm + xp;
    s = s + ym;
    s = s + yp;
    s = s + zm;
    s = s + zp;
    const float L = invdx2 * (s - 6.0f * p);
    return p + dt * L;
}

// The 12 edge neighbours of the curvature stencil, in the order the mixed differences read them: v(i,j,k) = val(c + (i,j,k))
struct Edges {
    float pp0, pm0, mm0, mp0;   // v(1,1,0)  v(1,-1,0)  v(-1,-1,0)  v(-1,1,0)
    float p0p, p0m, m0m, m0p;   // v(1,0,1)  v(1,0,-1)  v(-1,0,-1)  v(-1,0,1)
    float zpp, zpm, zmm, zmp;   // v(0,1,1)  v(0,1,-1)  v(0,-1,-1)  v(0,-1,1)
};

// CurvatureStencil::meanCurvatureNormGrad and the explicit step: differences in float, everything after them in double (the
// library's Real), the term narrowed once
FDEF float curvature_value(float p, float xm, float xp, float ym, float yp, float zm, float zp, const Edges& e, float invdx2, float dt)
{
    const double Dx = 0.5 * (double)(xp - xm), Dy = 0.5 * (double)(yp - ym), Dz = 0.5 * (double)(zp - zm);
    const double Dx2 = Dx * Dx, Dy2 = Dy * Dy, Dz2 = Dz * Dz;
    const double ng = (Dx2 + Dy2) + Dz2;
    float F = 0.0f;
    if (!(ng <= 1e-15)) {
        const double Dxx = (double)((xp - 2.0f * p) + xm), Dyy = (double)((yp - 2.0f * p) + ym), Dzz = (double)((zp - 2.0f * p) + zm);
        const double Dxy = 0.25 * (double)(((e.pp0 - e.pm0) + e.mm0) - e.mp0);
        const double Dxz = 0.25 * (double)(((e.p0p - e.p0m) + e.m0m) - e.m0p);
        const double Dyz = 0.25 * (double)(((e.zpp - e.zpm) + e.zmm) - e.zmp);
        const double alpha = ((Dx2 * (Dyy + Dzz) + Dy2 * (Dxx + Dzz)) + Dz2 * (Dxx + Dyy)) - 2.0 * ((Dx * ((Dy * Dxy) + (Dz * Dxz))) + ((Dy * Dz) * Dyz));
        const double beta = sqrt(ng);
        F = (float)((alpha * (double)invdx2) / (2.0 * (beta * beta)));
    }
    return p + dt * F;
}

// The median's order: the usual monotone 32-bit key of a float's bytes (all bits of a negative flipped, the sign bit of the
// others set); -0 sorts before +0 and equal keys are equal bytes.
FDEF uint32_t median_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
FDEF uint32_t median_bits(uint32_t key) { return (key & 0x80000000u) ? key & 0x7fffffffu : ~key; }
constexpr int median_count(int W) { return (2 * W + 1) * (2 * W + 1) * (2 * W + 1); }

// The key at zero-based rank `rank` of the m keys key(0) .. key(m - 1), by radix selection from the top bit down: 32 sweeps, no
// storage.  A function of the multiset alone.
template <typename Key> FDEF uint32_t median_select(int m, int rank, Key key)
{
    uint32_t prefix = 0;
    for (int b = 31; b >= 0; --b) {
        int below = 0;   // the keys that agree with the prefix above bit b and have bit b clear
#ifdef __HIPCC__
#pragma unroll   // (m is a constant in the kernel: the keys' places become immediate offsets)
#endif
        for (int i = 0; i < m; ++i) below += ((key(i) ^ prefix) >> b) == 0u;
        if (rank >= below) rank -= below, prefix |= 1u << b;
    }
    return prefix;
}

}  // namespace fdef
