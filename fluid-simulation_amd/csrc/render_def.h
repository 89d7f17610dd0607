// The per-pixel arithmetic of "liquid surface as an image" (include/fluid_hip.h), stated once for the kernel (kernels_render.hip,
// hipcc) and the host function (render_host.cpp, g++): limits, the pixel's ray, the trilinear value and the gradient of a cell's
// eight corners, the shade.  How the corners are fetched and which samples are looked at is each side's own.  Both builds state
// -ffp-contract=off; every product is formed before its sum.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/fluid_hip.h"

#ifdef __HIPCC__
#define RDEF __host__ __device__ __forceinline__
#else
#define RDEF inline
#endif

namespace rdef {

RDEF bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the limits of the definition: nullptr, or what is wrong
inline const char* check(const fluid_camera_t* c, const fluid_shade_t* sh, uint32_t what)
{
    if (!c) return "render: null camera";
    if (what == 0 || (what & ~(FLUID_RENDER_RGB | FLUID_RENDER_DEPTH | FLUID_RENDER_NORMALS))) return "render: `what` must name at least one of the three parts and nothing else";
    if (c->width < 1 || c->width > 8192 || c->height < 1 || c->height > 8192 || (int64_t)c->width * c->height > (1 << 24))
        return "render: width and height in 1..8192 and at most 2^24 pixels are required";
    if (c->n_steps < 1 || c->n_steps > 65536) return "render: n_steps in 1..65536 is required";
    if (!finite3(c->eye) || !finite3(c->dir00) || !finite3(c->du) || !finite3(c->dv) || !std::isfinite(c->t_near) || !std::isfinite(c->step))
        return "render: every camera float must be finite";
    if (!(c->step > 0.0f) || !(c->t_near >= 0.0f)) return "render: step > 0 and t_near >= 0 are required";
    if (sh && (!finite3(sh->base) || sh->pad_ != 0)) return "render: a finite base colour and pad_ == 0 are required";
    return nullptr;
}

inline fluid_shade_t default_shade()
{
    fluid_shade_t s{};
    s.base[0] = s.base[1] = s.base[2] = 1.0f;
    return s;
}

// bytes of a record's parts
inline size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }
inline size_t rgb_at() { return 16; }
inline size_t depth_at(size_t px, uint32_t what) { return 16 + ((what & FLUID_RENDER_RGB) ? pad16(3 * px) : 0); }
inline size_t normals_at(size_t px, uint32_t what) { return depth_at(px, what) + ((what & FLUID_RENDER_DEPTH) ? 4 * px : 0); }
inline size_t record_bytes(size_t px, uint32_t what) { return normals_at(px, what) + ((what & FLUID_RENDER_NORMALS) ? 12 * px : 0); }

// the unit direction of pixel (i, j); false: a miss
RDEF bool ray_dir(const fluid_camera_t& c, int i, int j, float* d)
{
    const float pi = (float)i + 0.5f, pj = (float)j + 0.5f;
    float D[3];
    for (int a = 0; a < 3; ++a) {
        const float u = pi * c.du[a];
        const float v = pj * c.dv[a];
        D[a] = (c.dir00[a] + u) + v;
    }
    float l2 = D[0] * D[0];
    l2 = l2 + D[1] * D[1];
    l2 = l2 + D[2] * D[2];
    const float len = sqrtf(l2);
    if (!(len > 0.0f) || !std::isfinite(len)) return false;
    for (int a = 0; a < 3; ++a) d[a] = D[a] / len;
    return true;
}

RDEF float sample_t(const fluid_camera_t& c, int k)
{
    const float ks = (float)k * c.step;
    return c.t_near + ks;
}

RDEF void point_at(const fluid_camera_t& c, const float* d, float t, float* p)
{
    for (int a = 0; a < 3; ++a) {
        const float td = t * d[a];
        p[a] = c.eye[a] + td;
    }
}

// the out-of-bounds rule of value(): false for a NaN too
RDEF bool in_bounds(const float* p, int lo, int hi)
{
    const float b0 = (float)(lo - 1), b1 = (float)(hi + 1);
    return p[0] >= b0 && p[0] < b1 && p[1] >= b0 && p[1] < b1 && p[2] >= b0 && p[2] < b1;
}

// cell and offset of an in-bounds point
RDEF void cell_of(const float* p, int* c, float* f)
{
    for (int a = 0; a < 3; ++a) {
        c[a] = (int)floorf(p[a]);
        f[a] = p[a] - (float)c[a];
    }
}

RDEF float lerp(float a, float b, float t)
{
    const float d = b - a;
    const float td = t * d;
    return a + td;
}

// v[dx * 4 + dy * 2 + dz]
RDEF float trilinear(const float* v, const float* f)
{
    const float z00 = lerp(v[0], v[1], f[2]), z01 = lerp(v[2], v[3], f[2]), z10 = lerp(v[4], v[5], f[2]), z11 = lerp(v[6], v[7], f[2]);
    const float y0 = lerp(z00, z01, f[1]), y1 = lerp(z10, z11, f[1]);
    return lerp(y0, y1, f[0]);
}

// the unit gradient of the trilinear interpolant ("normals and triangles"), +0 where it has no length
RDEF void normal_of(const float* v, const float* f, float* n)
{
    const float e[3] = {1.0f - f[0], 1.0f - f[1], 1.0f - f[2]};
    const int stride[3] = {4, 2, 1};
    float g[3];
    for (int a = 0; a < 3; ++a) {
        const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
        float s = 0.0f;
        for (int o = 0; o < 4; ++o) {
            const int d1 = o >> 1, d2 = o & 1;
            const float w = (d1 ? f[b1] : e[b1]) * (d2 ? f[b2] : e[b2]);
            const int i0 = d1 * stride[b1] + d2 * stride[b2];
            const float dv = v[i0 + stride[a]] - v[i0];
            const float wd = w * dv;
            s = s + wd;
        }
        g[a] = s;
    }
    float l2 = g[0] * g[0];
    l2 = l2 + g[1] * g[1];
    l2 = l2 + g[2] * g[2];
    const float len = sqrtf(l2);
    const bool some = len > 0.0f;
    for (int a = 0; a < 3; ++a) n[a] = some ? g[a] / len : 0.0f;
}

RDEF float hit_time(float t0, float t1, float v0, float v1)
{
    const float dt = t1 - t0;
    const float num = dt * v0;
    const float den = v0 - v1;
    return t0 + num / den;
}

RDEF void shade(const fluid_shade_t& sh, const float* n, const float* d, uint8_t* rgb)
{
    float s = n[0] * d[0];
    s = s + n[1] * d[1];
    s = s + n[2] * d[2];
    s = fabsf(s);
    for (int c = 0; c < 3; ++c) {
        float x = sh.base[c] * s;
        x = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
        const float y = x * 255.0f;
        rgb[c] = (uint8_t)(y + 0.5f);
    }
}

}  // namespace rdef
