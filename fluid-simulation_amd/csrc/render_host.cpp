// The liquid surface as an image on the host (include/fluid_hip.h, "liquid surface as an image") — no GPU, no HIP, no OpenVDB.
//   fluid_sdf_render      the definition applied to a leaf list, every unlisted leaf being +bg: how a block run renders (after
//                         fluid_sdf_grids_merge and fluid_sdf_filter), and the second implementation the kernels
//                         (kernels_render.hip) are compared with.  Every sample of every ray is evaluated — nothing is skipped —,
//                         a cell's corners come from up to eight leaves found by bisection (leaf_list.h); no dense grid.
//   fluid_camera_look_at  a pinhole camera in double, narrowed once.
//   fluid_write_png       8-bit RGB, filter 0, one IDAT through zlib.
// Arithmetic: render_def.h, float, no contraction (the Makefile and the sanitizer build state -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <zlib.h>

#include "leaf_list.h"
#include "render_def.h"

namespace {

struct Caster {
    const fluid_sdf_grid_t* g;
    int lo, hi;
    float bg;
    // the leaf that was looked up last: neighbouring samples ask for the same leaves
    mutable Org last_o{0, 0, 0};
    mutable long last_l = -2;

    float val(int x, int y, int z) const
    {
        if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) return bg;
        const Org o{floor_to(x, LEAF), floor_to(y, LEAF), floor_to(z, LEAF)};
        if (last_l == -2 || !(o == last_o)) last_o = o, last_l = find_leaf(g, o);
        if (last_l < 0) return bg;
        return g->values[512 * (size_t)last_l + (((x & 7) * 8 + (y & 7)) * 8 + (z & 7))];
    }
    void corners(const int* c, float* v) const
    {
        for (int d = 0; d < 8; ++d) v[d] = val(c[0] + (d >> 2), c[1] + ((d >> 1) & 1), c[2] + (d & 1));
    }
    float value(const float* p) const
    {
        if (!rdef::in_bounds(p, lo, hi)) return bg;
        int c[3];
        float f[3], v[8];
        rdef::cell_of(p, c, f);
        corners(c, v);
        return rdef::trilinear(v, f);
    }
};

void put_u32(std::vector<uint8_t>& b, uint32_t v)
{
    for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)(v >> s));
}

// length, type, data, crc of type and data
bool write_chunk(FILE* f, const char* type, const uint8_t* data, size_t n)
{
    std::vector<uint8_t> head;
    put_u32(head, (uint32_t)n);
    head.insert(head.end(), type, type + 4);
    uLong crc = crc32(0L, (const Bytef*)type, 4);
    if (n) crc = crc32(crc, (const Bytef*)data, (uInt)n);
    std::vector<uint8_t> tail;
    put_u32(tail, (uint32_t)crc);
    return fwrite(head.data(), 1, 8, f) == 8 && (n == 0 || fwrite(data, 1, n, f) == n) && fwrite(tail.data(), 1, 4, f) == 4;
}

}  // namespace

extern "C" {

int fluid_sdf_render(const fluid_sdf_grid_t* g, const fluid_camera_t* cam, const fluid_shade_t* shade, uint32_t what, uint8_t* rgb, float* depth,
                     float* normals, int64_t* n_hit)
{
    if (check_list(g) != FLUID_OK || rdef::check(cam, shade, what)) return FLUID_ERR_ARG;
    if (((what & FLUID_RENDER_RGB) && !rgb) || ((what & FLUID_RENDER_DEPTH) && !depth) || ((what & FLUID_RENDER_NORMALS) && !normals)) return FLUID_ERR_ARG;
    const fluid_shade_t sh = shade ? *shade : rdef::default_shade();
    const fluid_camera_t& c = *cam;
    Caster ca;
    ca.g = g;
    ca.lo = -(g->n / 2), ca.hi = ca.lo + g->n - 1;
    ca.bg = g->background;
    int64_t hits = 0;
    for (int j = 0; j < c.height; ++j)
        for (int i = 0; i < c.width; ++i) {
            const size_t at = (size_t)j * c.width + i;
            float d[3], t = INFINITY, n[3] = {0.0f, 0.0f, 0.0f};
            bool hit = false;
            if (rdef::ray_dir(c, i, j, d)) {
                float t0 = 0.0f, v0 = 0.0f;
                for (int k = 0; k < c.n_steps; ++k) {
                    const float tk = rdef::sample_t(c, k);
                    float p[3];
                    rdef::point_at(c, d, tk, p);
                    const float v1 = ca.value(p);
                    if (v1 < 0.0f) {
                        t = k == 0 ? tk : rdef::hit_time(t0, tk, v0, v1);
                        hit = true;
                        break;
                    }
                    t0 = tk, v0 = v1;
                }
            }
            if (hit) {
                ++hits;
                float ph[3];
                rdef::point_at(c, d, t, ph);
                if (rdef::in_bounds(ph, ca.lo, ca.hi)) {
                    int cc[3];
                    float f[3], v[8];
                    rdef::cell_of(ph, cc, f);
                    ca.corners(cc, v);
                    rdef::normal_of(v, f, n);
                }
            }
            if (what & FLUID_RENDER_RGB) {
                if (hit) rdef::shade(sh, n, d, rgb + 3 * at);
                else memcpy(rgb + 3 * at, sh.background, 3);
            }
            if (what & FLUID_RENDER_DEPTH) depth[at] = t;
            if (what & FLUID_RENDER_NORMALS) memcpy(normals + 3 * at, n, sizeof n);
        }
    if (n_hit) *n_hit = hits;
    return FLUID_OK;
}

int fluid_camera_look_at(int32_t n, const double eye[3], const double target[3], const double up[3], double fov_y_degrees, int32_t width, int32_t height,
                         double step, fluid_camera_t* out)
{
    if (!eye || !target || !up || !out || n < 1 || width < 1 || width > 8192 || height < 1 || height > 8192 || (int64_t)width * height > (1 << 24))
        return FLUID_ERR_ARG;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(eye[a]) || !std::isfinite(target[a]) || !std::isfinite(up[a])) return FLUID_ERR_ARG;
    if (!(fov_y_degrees > 0.0) || !(fov_y_degrees < 180.0) || !(step > 0.0) || !std::isfinite(step) || !((float)step > 0.0f)) return FLUID_ERR_ARG;
    auto norm = [](double* v) {
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(l > 0.0) || !std::isfinite(l)) return false;
        for (int a = 0; a < 3; ++a) v[a] /= l;
        return true;
    };
    double fw[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]}, u[3] = {up[0], up[1], up[2]};
    if (!norm(fw) || !norm(u)) return FLUID_ERR_ARG;
    double rt[3] = {fw[1] * u[2] - fw[2] * u[1], fw[2] * u[0] - fw[0] * u[2], fw[0] * u[1] - fw[1] * u[0]};   // forward x up
    if (!(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2] > 1e-12) || !norm(rt)) return FLUID_ERR_ARG;   // up within 1e-6 rad of the view
    const double dn[3] = {fw[1] * rt[2] - fw[2] * rt[1], fw[2] * rt[0] - fw[0] * rt[2], fw[0] * rt[1] - fw[1] * rt[0]};   // forward x right: down the image
    const double half_h = std::tan(fov_y_degrees * (3.14159265358979323846 / 360.0));
    const double px = 2.0 * half_h / height;   // a pixel's size on the plane at distance 1
    fluid_camera_t c{};
    for (int a = 0; a < 3; ++a) {
        c.eye[a] = (float)eye[a];
        c.du[a] = (float)(px * rt[a]);
        c.dv[a] = (float)(px * dn[a]);
        c.dir00[a] = (float)(fw[a] - 0.5 * width * px * rt[a] - 0.5 * height * px * dn[a]);
    }
    c.width = width, c.height = height;
    c.t_near = 0.0f;
    c.step = (float)step;
    // the farthest corner of the box the definition can give a value in, [lo - 1, hi + 1]^3
    const double lo = -(n / 2) - 1.0, hi = -(n / 2) + n + 0.0;
    double far2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double m = std::fmax(std::fabs(eye[a] - lo), std::fabs(eye[a] - hi));
        far2 += m * m;
    }
    const double ks = std::ceil(std::sqrt(far2) / (double)c.step) + 2.0;
    c.n_steps = ks > 65536.0 ? 65536 : (int32_t)ks;
    *out = c;
    return FLUID_OK;
}

int fluid_write_png(const char* path, int32_t width, int32_t height, const uint8_t* rgb)
{
    if (!path || !rgb || width < 1 || width > 8192 || height < 1 || height > 8192) return FLUID_ERR_ARG;
    const size_t row = 3 * (size_t)width;
    std::vector<uint8_t> raw((row + 1) * (size_t)height);
    for (int j = 0; j < height; ++j) {
        raw[(row + 1) * j] = 0;   // filter type 0
        memcpy(raw.data() + (row + 1) * j + 1, rgb + row * j, row);
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), 6) != Z_OK) return FLUID_ERR_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return FLUID_ERR_ARG;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<uint8_t> ihdr;
    put_u32(ihdr, (uint32_t)width);
    put_u32(ihdr, (uint32_t)height);
    const uint8_t rest[5] = {8, 2, 0, 0, 0};   // bit depth, colour type RGB, compression, filter, interlace
    ihdr.insert(ihdr.end(), rest, rest + 5);
    bool ok = fwrite(sig, 1, 8, f) == 8 && write_chunk(f, "IHDR", ihdr.data(), ihdr.size()) && write_chunk(f, "IDAT", z.data(), zn) &&
              write_chunk(f, "IEND", nullptr, 0);
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        remove(path);
        return FLUID_ERR_ARG;
    }
    return FLUID_OK;
}

}  // extern "C"
