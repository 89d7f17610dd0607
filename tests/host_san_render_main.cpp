// fluid_sdf_render, fluid_camera_look_at and fluid_write_png under AddressSanitizer + UBSan (tests/test_render_sanitizers.py builds and
// runs this with g++ together with render_host.cpp and vdb_sdf_writer.cpp): a hand-made leaf list — two balls, one cut by the grid's
// corner, in a grid whose first and last leaves are partial (n = 24) — seen by cameras outside, inside the liquid, along the axes in
// leaf faces, with steps that run far out of bounds and with no direction at all; every image against the definition restated here
// on the dense array fluid_sdf_to_dense gives (another way to the corners than the bisection), bit for bit; every refused kind of
// input; a PNG written, re-read and refused.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fluid_hip.h"

static int fail(const char* what)
{
    std::fprintf(stderr, "FAILED: %s\n", what);
    return 1;
}

static const int N = 24, LO = -12, HI = 11, L0 = -16;
static const float BG = 2.0f;

static float ball(int x, int y, int z)
{
    const float a = std::sqrt((float)((x - 1) * (x - 1) + (y + 2) * (y + 2) + z * z)) - 3.5f;
    const float b = std::sqrt((float)((x - 11) * (x - 11) + (y - 11) * (y - 11) + (z - 11) * (z - 11))) - 4.0f;
    const float d = a < b ? a : b;
    return d > BG ? BG : (d < -BG ? -BG : d);
}

struct Dense {
    std::vector<float> v;
    float at(int x, int y, int z) const
    {
        if (x < LO || x > HI || y < LO || y > HI || z < LO || z > HI) return BG;
        return v[((size_t)(x - LO) * N + (y - LO)) * N + (z - LO)];
    }
    static bool inb(const float* p)
    {
        for (int a = 0; a < 3; ++a)
            if (!(p[a] >= (float)(LO - 1) && p[a] < (float)(HI + 1))) return false;
        return true;
    }
    void cell(const float* p, float* c8, float* f) const
    {
        int c[3];
        for (int a = 0; a < 3; ++a) c[a] = (int)std::floor(p[a]), f[a] = p[a] - (float)c[a];
        for (int d = 0; d < 8; ++d) c8[d] = at(c[0] + (d >> 2), c[1] + ((d >> 1) & 1), c[2] + (d & 1));
    }
    static float lerp(float a, float b, float t)
    {
        volatile float d = b - a;
        volatile float td = t * d;
        return a + td;
    }
    float value(const float* p) const
    {
        if (!inb(p)) return BG;
        float c[8], f[3];
        cell(p, c, f);
        const float z0 = lerp(c[0], c[1], f[2]), z1 = lerp(c[2], c[3], f[2]), z2 = lerp(c[4], c[5], f[2]), z3 = lerp(c[6], c[7], f[2]);
        return lerp(lerp(z0, z1, f[1]), lerp(z2, z3, f[1]), f[0]);
    }
};

// the definition, pixel by pixel (volatile keeps every product apart from its sum whatever the flags)
static void restate(const Dense& D, const fluid_camera_t& c, const fluid_shade_t& sh, std::vector<uint8_t>& rgb, std::vector<float>& depth,
                    std::vector<float>& nrm, int64_t& hits)
{
    const size_t px = (size_t)c.width * c.height;
    rgb.assign(3 * px, 0), depth.assign(px, 0.0f), nrm.assign(3 * px, 0.0f);
    hits = 0;
    for (int j = 0; j < c.height; ++j)
        for (int i = 0; i < c.width; ++i) {
            const size_t at = (size_t)j * c.width + i;
            const float pi = (float)i + 0.5f, pj = (float)j + 0.5f;
            float Dv[3], d[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                volatile float u = pi * c.du[a], v = pj * c.dv[a];
                Dv[a] = (c.dir00[a] + u) + v;
            }
            volatile float q0 = Dv[0] * Dv[0], q1 = Dv[1] * Dv[1], q2 = Dv[2] * Dv[2];
            volatile float l2 = q0;
            l2 = l2 + q1;
            l2 = l2 + q2;
            const float len = std::sqrt(l2);
            float t = INFINITY, n[3] = {0, 0, 0};
            bool hit = false;
            if (len > 0.0f && std::isfinite(len)) {
                for (int a = 0; a < 3; ++a) d[a] = Dv[a] / len;
                float t0 = 0, v0 = 0;
                for (int k = 0; k < c.n_steps && !hit; ++k) {
                    volatile float ks = (float)k * c.step;
                    const float tk = c.t_near + ks;
                    float p[3];
                    for (int a = 0; a < 3; ++a) {
                        volatile float td = tk * d[a];
                        p[a] = c.eye[a] + td;
                    }
                    const float v1 = D.value(p);
                    if (v1 < 0.0f) {
                        hit = true;
                        if (k == 0) t = tk;
                        else {
                            volatile float dt = tk - t0;
                            volatile float num = dt * v0;
                            volatile float den = v0 - v1;
                            volatile float quo = num / den;
                            t = t0 + quo;
                        }
                    }
                    t0 = tk, v0 = v1;
                }
            }
            if (hit) {
                ++hits;
                float p[3];
                for (int a = 0; a < 3; ++a) {
                    volatile float td = t * d[a];
                    p[a] = c.eye[a] + td;
                }
                if (Dense::inb(p)) {
                    float c8[8], f[3], g[3];
                    D.cell(p, c8, f);
                    const float e[3] = {1.0f - f[0], 1.0f - f[1], 1.0f - f[2]};
                    const int stride[3] = {4, 2, 1};
                    for (int a = 0; a < 3; ++a) {
                        const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
                        volatile float s = 0.0f;
                        for (int o = 0; o < 4; ++o) {
                            const int d1 = o >> 1, d2 = o & 1, i0 = d1 * stride[b1] + d2 * stride[b2];
                            volatile float w = (d1 ? f[b1] : e[b1]) * (d2 ? f[b2] : e[b2]);
                            volatile float dv = c8[i0 + stride[a]] - c8[i0];
                            volatile float wd = w * dv;
                            s = s + wd;
                        }
                        g[a] = s;
                    }
                    volatile float g0 = g[0] * g[0], g1 = g[1] * g[1], g2 = g[2] * g[2];
                    volatile float m2 = g0;
                    m2 = m2 + g1;
                    m2 = m2 + g2;
                    const float gl = std::sqrt(m2);
                    for (int a = 0; a < 3; ++a) n[a] = gl > 0.0f ? g[a] / gl : 0.0f;
                }
            }
            depth[at] = t;
            memcpy(&nrm[3 * at], n, sizeof n);
            if (!hit) memcpy(&rgb[3 * at], sh.background, 3);
            else {
                volatile float s0 = n[0] * d[0], s1 = n[1] * d[1], s2 = n[2] * d[2];
                volatile float s = s0;
                s = s + s1;
                s = s + s2;
                const float sa = std::fabs(s);
                for (int ch = 0; ch < 3; ++ch) {
                    volatile float x = sh.base[ch] * sa;
                    const float xc = x > 0.0f ? (x < 1.0f ? (float)x : 1.0f) : 0.0f;
                    volatile float y = xc * 255.0f;
                    rgb[3 * at + ch] = (uint8_t)(y + 0.5f);
                }
            }
        }
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    // the list: every leaf that holds a value other than +BG, ascending; voxels outside the grid are +BG
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
    for (int ox = L0; ox <= (HI & ~7); ox += 8)
        for (int oy = L0; oy <= (HI & ~7); oy += 8)
            for (int oz = L0; oz <= (HI & ~7); oz += 8) {
                float v[512];
                uint64_t m[8] = {};
                bool any = false;
                for (int off = 0; off < 512; ++off) {
                    const int x = ox + (off >> 6), y = oy + ((off >> 3) & 7), z = oz + (off & 7);
                    const bool in = x >= LO && x <= HI && y >= LO && y <= HI && z >= LO && z <= HI;
                    v[off] = in ? ball(x, y, z) : BG;
                    if (v[off] > -BG && v[off] < BG) m[off >> 6] |= 1ull << (off & 63);
                    any = any || v[off] != BG;
                }
                if (!any) continue;
                origin.insert(origin.end(), {ox, oy, oz});
                values.insert(values.end(), v, v + 512);
                active.insert(active.end(), m, m + 8);
            }
    fluid_sdf_grid_t g{N, (int32_t)(origin.size() / 3), BG, 3.5f, 2.0f, origin.data(), values.data(), active.data()};
    if (g.n_leaves < 8 || g.n_leaves >= 64) return fail("the list should hold some leaves, not all");
    Dense D;
    D.v.resize((size_t)N * N * N);
    if (fluid_sdf_to_dense(&g, D.v.data(), nullptr) != FLUID_OK) return fail("fluid_sdf_to_dense");

    std::vector<fluid_camera_t> cams;
    const double target[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    fluid_camera_t c{};
    const double eyes[3][3] = {{-25, 12, -30}, {1, -2, 0.25}, {30, 30, 30}};   // outside; inside the first ball; beyond the cut ball
    for (int k = 0; k < 3; ++k) {
        if (fluid_camera_look_at(N, eyes[k], target, up, k == 1 ? 90.0 : 35.0, 23, 17, 0.5, &c) != FLUID_OK) return fail("fluid_camera_look_at");
        if (c.width != 23 || c.height != 17 || c.t_near != 0.0f || c.step != 0.5f || c.n_steps < 40 || c.n_steps > 400) return fail("look_at's record");
        cams.push_back(c);
    }
    c.step = 1e3f, c.n_steps = 65536, c.width = 3, c.height = 2;   // far out of bounds
    cams.push_back(c);
    for (int a = 0; a < 3; ++a)
        for (int sgn = -1; sgn <= 1; sgn += 2) {   // along the axes, in the leaf faces x, y or z = 0 and 8
            fluid_camera_t o{};
            o.eye[a] = sgn > 0 ? -24.0f : 24.0f, o.eye[(a + 1) % 3] = 0.0f, o.eye[(a + 2) % 3] = sgn > 0 ? 0.0f : 8.0f;
            o.dir00[a] = (float)sgn;
            o.width = 2, o.height = 1, o.step = 0.5f, o.n_steps = 100;
            cams.push_back(o);
        }
    fluid_camera_t none = cams[1];   // no direction: every pixel a miss, even with the eye in the liquid
    for (int a = 0; a < 3; ++a) none.dir00[a] = none.du[a] = none.dv[a] = 0.0f;
    cams.push_back(none);

    const fluid_shade_t sh{{0.9f, 0.5f, 1.7f}, {3, 200, 77}, 0};
    int64_t all_hits = 0;
    for (size_t k = 0; k < cams.size(); ++k) {
        const fluid_camera_t& cam = cams[k];
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<uint8_t> rgb(3 * px), rrgb;
        std::vector<float> depth(px), nrm(3 * px), rdepth, rnrm;
        int64_t hits = -1, rhits = -1;
        if (fluid_sdf_render(&g, &cam, &sh, 7, rgb.data(), depth.data(), nrm.data(), &hits) != FLUID_OK) return fail("fluid_sdf_render");
        restate(D, cam, sh, rrgb, rdepth, rnrm, rhits);
        if (hits != rhits || rgb != rrgb || memcmp(depth.data(), rdepth.data(), 4 * px) || memcmp(nrm.data(), rnrm.data(), 12 * px)) {
            std::fprintf(stderr, "camera %zu: hits %lld / %lld\n", k, (long long)hits, (long long)rhits);
            return fail("fluid_sdf_render differs from the definition");
        }
        if (k == 1 && hits != (int64_t)px) return fail("an eye in the liquid hits everywhere");
        if (k == cams.size() - 1 && hits != 0) return fail("no direction, no hit");
        all_hits += hits;
        // each part alone, exact-size arrays: nothing beyond them is touched
        for (uint32_t what = 1; what < 7; ++what) {
            std::vector<uint8_t> r1((what & 1) ? 3 * px : 0);
            std::vector<float> d1((what & 2) ? px : 0), n1((what & 4) ? 3 * px : 0);
            if (fluid_sdf_render(&g, &cam, nullptr, what, (what & 1) ? r1.data() : nullptr, (what & 2) ? d1.data() : nullptr, (what & 4) ? n1.data() : nullptr,
                                 nullptr) != FLUID_OK)
                return fail("fluid_sdf_render with a choice of parts");
            if ((what & 2) && memcmp(d1.data(), depth.data(), 4 * px)) return fail("depth alone");
            if ((what & 4) && memcmp(n1.data(), nrm.data(), 12 * px)) return fail("normals alone");
        }
    }
    if (all_hits < 100) return fail("the cameras should see the balls");
    // an empty list: all misses
    {
        fluid_sdf_grid_t e{N, 0, BG, 3.5f, 2.0f, nullptr, nullptr, nullptr};
        std::vector<float> depth((size_t)cams[0].width * cams[0].height);
        int64_t hits = -1;
        if (fluid_sdf_render(&e, &cams[0], nullptr, FLUID_RENDER_DEPTH, nullptr, depth.data(), nullptr, &hits) != FLUID_OK || hits != 0) return fail("empty list");
        for (float t : depth)
            if (!(std::isinf(t) && t > 0)) return fail("a miss is +infinity");
    }
    // refusals
    {
        uint8_t px3[3];
        float one[3];
        fluid_camera_t tiny = cams[0];
        tiny.width = tiny.height = 1;
        auto refused = [&](const fluid_sdf_grid_t* gg, const fluid_camera_t* cc, const fluid_shade_t* ss, uint32_t what, uint8_t* r, float* d, float* n) {
            return fluid_sdf_render(gg, cc, ss, what, r, d, n, nullptr) == FLUID_ERR_ARG;
        };
        if (fluid_sdf_render(&g, &tiny, &sh, 7, px3, one, one, nullptr) != FLUID_OK) return fail("1 x 1");
        fluid_camera_t b = tiny;
        b.width = 0;
        if (!refused(&g, &b, &sh, 7, px3, one, one)) return fail("width 0");
        b = tiny, b.n_steps = 65537;
        if (!refused(&g, &b, &sh, 7, px3, one, one)) return fail("n_steps");
        b = tiny, b.step = NAN;
        if (!refused(&g, &b, &sh, 7, px3, one, one)) return fail("step NaN");
        b = tiny, b.t_near = -1.0f;
        if (!refused(&g, &b, &sh, 7, px3, one, one)) return fail("t_near");
        b = tiny, b.du[1] = INFINITY;
        if (!refused(&g, &b, &sh, 7, px3, one, one)) return fail("du infinite");
        fluid_shade_t bs = sh;
        bs.pad_ = 1;
        if (!refused(&g, &tiny, &bs, 7, px3, one, one)) return fail("pad_");
        if (!refused(&g, &tiny, &sh, 0, px3, one, one) || !refused(&g, &tiny, &sh, 8, px3, one, one)) return fail("what");
        if (!refused(&g, &tiny, &sh, 7, nullptr, one, one) || !refused(&g, &tiny, &sh, 7, px3, nullptr, one) || !refused(&g, &tiny, &sh, 7, px3, one, nullptr)) return fail("a part without its array");
        if (!refused(nullptr, &tiny, &sh, 7, px3, one, one) || !refused(&g, nullptr, &sh, 7, px3, one, one)) return fail("null");
        std::vector<int32_t> o2 = origin;
        std::swap(o2[0], o2[3]), std::swap(o2[1], o2[4]), std::swap(o2[2], o2[5]);   // not ascending
        fluid_sdf_grid_t g2 = g;
        g2.origin = o2.data();
        if (!refused(&g2, &tiny, &sh, 7, px3, one, one)) return fail("a list that is not ascending");
        const double same[3] = {-25, 12, -30}, above[3] = {0, 9, 0};
        if (fluid_camera_look_at(N, same, same, up, 40.0, 4, 4, 0.5, &b) != FLUID_ERR_ARG || fluid_camera_look_at(N, above, target, up, 40.0, 4, 4, 0.5, &b) != FLUID_ERR_ARG ||
            fluid_camera_look_at(N, same, target, up, 180.0, 4, 4, 0.5, &b) != FLUID_ERR_ARG || fluid_camera_look_at(N, same, target, up, 40.0, 4, 4, 0.0, &b) != FLUID_ERR_ARG ||
            fluid_camera_look_at(N, same, target, up, 40.0, 0, 4, 0.5, &b) != FLUID_ERR_ARG || fluid_camera_look_at(0, same, target, up, 40.0, 4, 4, 0.5, &b) != FLUID_ERR_ARG)
            return fail("fluid_camera_look_at's refusals");
    }
    // PNG: written in full, the signature and the three chunks where they belong; a path that cannot be opened leaves nothing
    {
        const fluid_camera_t& cam = cams[0];
        std::vector<uint8_t> rgb(3 * (size_t)cam.width * cam.height);
        if (fluid_sdf_render(&g, &cam, &sh, 1, rgb.data(), nullptr, nullptr, nullptr) != FLUID_OK) return fail("render for the PNG");
        const std::string path = dir + "/frame.png";
        if (fluid_write_png(path.c_str(), cam.width, cam.height, rgb.data()) != FLUID_OK) return fail("fluid_write_png");
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return fail("the PNG is not there");
        std::vector<uint8_t> raw(1 << 20);
        raw.resize(fread(raw.data(), 1, raw.size(), f));
        fclose(f);
        static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        if (raw.size() < 57 || memcmp(raw.data(), sig, 8) || memcmp(&raw[12], "IHDR", 4) || memcmp(&raw[37], "IDAT", 4) || memcmp(&raw[raw.size() - 8], "IEND", 4))
            return fail("the PNG's layout");
        if (raw[16 + 3] != 23 || raw[20 + 3] != 17 || raw[24] != 8 || raw[25] != 2) return fail("the PNG's header");
        if (fluid_write_png((dir + "/no/such/dir.png").c_str(), 2, 2, rgb.data()) != FLUID_ERR_ARG) return fail("a path that cannot be opened");
        if (fluid_write_png(path.c_str(), 0, 2, rgb.data()) != FLUID_ERR_ARG || fluid_write_png(path.c_str(), 2, 2, nullptr) != FLUID_ERR_ARG ||
            fluid_write_png(nullptr, 2, 2, rgb.data()) != FLUID_ERR_ARG)
            return fail("fluid_write_png's refusals");
    }
    std::printf("render: %d leaves, %zu cameras, %lld hits\n", g.n_leaves, cams.size(), (long long)all_hits);
    std::printf("host sanitizer run: ok\n");
    return 0;
}
