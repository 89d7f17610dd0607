// fluid_particles_trails and fluid_spheres_surface under AddressSanitizer + UBSan (tests/test_sdf_trail_host.py builds and runs this
// with g++ together with sdf_trail_host.cpp): a filled block beside scattered particles, some outside the grid, one NaN position and
// velocities that are zero, NaN, infinite and huge, on n = 9 (odd: a partial last cell row) and n = 16; an exact capacity and one too
// small; the promises of the definition (a trail never takes liquid away from the spheres); refused arguments.  The instances and
// the grids are written to <dir>/san_trail_<n>.bin for the test to compare with the library's own bytes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fluid_hip.h"

static int fail(const char* what)
{
    std::fprintf(stderr, "FAILED: %s\n", what);
    return 1;
}

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double uni(uint32_t& s, double a, double b) { return a + (b - a) * ((rnd(s) >> 8) / 16777216.0); }

// the same particles as tests/test_sdf_trail_host.py::san_particles makes (same generator, same order)
static void particles(int n, std::vector<double>& p, std::vector<double>& v)
{
    const int lo = -(n / 2), hi = lo + n - 1;
    uint32_t s = 4048u + (uint32_t)n;
    for (int x = -2; x < 2; ++x)
        for (int y = -2; y < 2; ++y)
            for (int z = -2; z < 2; ++z)
                for (int k = 0; k < 2; ++k) {
                    for (int c : {x, y, z}) p.push_back(c + uni(s, -0.5, 0.5));
                    for (int a = 0; a < 3; ++a) v.push_back(uni(s, -1.0, 1.0));
                }
    for (int i = 0; i < 60; ++i) {
        for (int a = 0; a < 3; ++a) p.push_back(uni(s, lo - 3.0, hi + 3.0));
        for (int a = 0; a < 3; ++a) v.push_back(uni(s, -6.0, 6.0));
    }
    p.insert(p.end(), {NAN, 0.0, 0.0}), v.insert(v.end(), {1.0, 0.0, 0.0});
    p.insert(p.end(), {1.0, 1.0, 1.0}), v.insert(v.end(), {NAN, 0.0, 0.0});
    p.insert(p.end(), {-1.0, 1.0, 1.0}), v.insert(v.end(), {INFINITY, 0.0, 0.0});
    p.insert(p.end(), {1.0, -1.0, 1.0}), v.insert(v.end(), {1e300, -1e300, 0.0});
    p.insert(p.end(), {1.0, 1.0, -1.0}), v.insert(v.end(), {0.0, 0.0, 0.0});
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const fluid_sdf_params_t prm = {1.5, 2.5};
    const fluid_sdf_trails_t tr = {1.0, 1.0, 0.5, 8, 0};
    for (int n : {9, 16}) {
        std::vector<double> p, v;
        particles(n, p, v);
        const int64_t np = (int64_t)(p.size() / 3);
        const size_t nc = (size_t)n * n * n;
        const int64_t k = fluid_particles_trails(np, p.data(), v.data(), &prm, &tr, 0, nullptr, nullptr);
        if (k < np + 60 || k > 8 * np) return fail("instance count");
        std::vector<double> ip((size_t)3 * k);   // exactly k: one slot more written is the sanitizer's to find
        std::vector<float> ir((size_t)k);
        if (fluid_particles_trails(np, p.data(), v.data(), &prm, &tr, k, ip.data(), ir.data()) != k) return fail("expansion");
        if (fluid_particles_trails(np, p.data(), v.data(), &prm, &tr, k - 1, ip.data(), ir.data()) != -FLUID_ERR_ARG) return fail("cap too small accepted");
        for (int64_t i = 0; i < k; ++i)
            if (!(ir[(size_t)i] > 0.0f && ir[(size_t)i] <= 1.5f)) return fail("a radius outside (0, R]");
        if (fluid_particles_trails(np, p.data(), nullptr, &prm, &tr, 0, nullptr, nullptr) != np) return fail("no velocities: one instance each");
        std::vector<float> vt(nc), vs(nc), v0(nc);
        std::vector<uint8_t> at(nc), as(nc);
        if (fluid_spheres_surface(n, 1.0, k, ip.data(), ir.data(), &prm, vt.data(), at.data()) != FLUID_OK) return fail("trails");
        if (fluid_spheres_surface(n, 1.0, k, ip.data(), ir.data(), &prm, v0.data(), nullptr) != FLUID_OK) return fail("trails, no mask");
        if (std::memcmp(vt.data(), v0.data(), nc * 4) != 0) return fail("the mask changes the values");
        std::vector<float> rs((size_t)np, 1.5f);
        if (fluid_spheres_surface(n, 1.0, np, p.data(), rs.data(), &prm, vs.data(), as.data()) != FLUID_OK) return fail("spheres");
        size_t active = 0, differ = 0;
        for (size_t c = 0; c < nc; ++c) {
            if (vt[c] > vs[c]) return fail("a trail took liquid away");   // instance 0 is the sphere itself
            active += at[c], differ += std::memcmp(&vt[c], &vs[c], 4) != 0;
        }
        if (!active || !differ) return fail("the trails' surface is empty or is the spheres'");
        const std::string path = dir + "/san_trail_" + std::to_string(n) + ".bin";
        std::FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(ip.data(), 8, (size_t)3 * k, f) != (size_t)3 * k || std::fwrite(ir.data(), 4, (size_t)k, f) != (size_t)k ||
            std::fwrite(vt.data(), 4, nc, f) != nc || std::fwrite(at.data(), 1, nc, f) != nc || std::fclose(f) != 0)
            return fail("write");
    }
    std::vector<float> val(512);
    const double one[3] = {0.0, 0.0, 0.0}, vel[3] = {2.0, 0.0, 0.0};
    const float r1 = 1.0f;
    const fluid_sdf_trails_t bad[] = {{-1.0, 1.0, 0.5, 8, 0}, {NAN, 1.0, 0.5, 8, 0}, {INFINITY, 1.0, 0.5, 8, 0}, {1.0, 0.0, 0.5, 8, 0}, {1.0, NAN, 0.5, 8, 0},
                                      {1.0, INFINITY, 0.5, 8, 0}, {1.0, 1.0, 0.0, 8, 0}, {1.0, 1.0, NAN, 8, 0}, {1.0, 1.0, 0.5, 0, 0}, {1.0, 1.0, 0.5, 33, 0},
                                      {1.0, 1.0, 0.5, 8, 1}, {1.0, 1.0, 1.6, 8, 0}};
    for (const fluid_sdf_trails_t& b : bad)
        if (fluid_particles_trails(1, one, vel, &prm, &b, 0, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("a bad setting accepted");
    const fluid_sdf_trails_t edge = {0.0, 1e300, 1.5, 32, 0};
    if (fluid_particles_trails(1, one, vel, &prm, &edge, 0, nullptr, nullptr) != 1) return fail("the limits themselves refused");
    const fluid_sdf_params_t wide = {2.0, 2.5};
    double op[3];
    float orad[1];
    if (fluid_particles_trails(1, one, vel, &wide, &tr, 0, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("R + w > 4 accepted");
    if (fluid_particles_trails(-1, one, vel, &prm, &tr, 0, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("np < 0 accepted");
    if (fluid_particles_trails(1, nullptr, vel, &prm, &tr, 0, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("NULL positions accepted");
    if (fluid_particles_trails(1, one, vel, nullptr, &tr, 0, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("NULL parameters accepted");
    if (fluid_particles_trails(1, one, vel, &prm, nullptr, 0, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("NULL setting accepted");
    if (fluid_particles_trails(1, one, vel, &prm, &tr, 8, op, nullptr) != -FLUID_ERR_ARG) return fail("one output alone accepted");
    if (fluid_particles_trails(1, one, vel, &prm, &tr, 8, nullptr, orad) != -FLUID_ERR_ARG) return fail("one output alone accepted");
    if (fluid_particles_trails(0, nullptr, nullptr, &prm, &tr, 0, nullptr, nullptr) != 0) return fail("no particles");
    for (float r : {0.0f, -1.0f, 1.6f, NAN, INFINITY})
        if (fluid_spheres_surface(8, 1.0, 1, one, &r, &prm, val.data(), nullptr) != FLUID_ERR_ARG) return fail("a bad radius accepted");
    if (fluid_spheres_surface(8, 1.0, 1, one, &r1, &wide, val.data(), nullptr) != FLUID_ERR_ARG) return fail("R + w > 4 accepted");
    if (fluid_spheres_surface(0, 1.0, 1, one, &r1, &prm, val.data(), nullptr) != FLUID_ERR_ARG) return fail("n = 0 accepted");
    if (fluid_spheres_surface(8, 0.0, 1, one, &r1, &prm, val.data(), nullptr) != FLUID_ERR_ARG) return fail("dx = 0 accepted");
    if (fluid_spheres_surface(8, 1.0, -1, one, &r1, &prm, val.data(), nullptr) != FLUID_ERR_ARG) return fail("n_items < 0 accepted");
    if (fluid_spheres_surface(8, 1.0, 1, nullptr, &r1, &prm, val.data(), nullptr) != FLUID_ERR_ARG) return fail("NULL positions accepted");
    if (fluid_spheres_surface(8, 1.0, 1, one, nullptr, &prm, val.data(), nullptr) != FLUID_ERR_ARG) return fail("NULL radii accepted");
    if (fluid_spheres_surface(8, 1.0, 1, one, &r1, nullptr, val.data(), nullptr) != FLUID_ERR_ARG) return fail("NULL parameters accepted");
    if (fluid_spheres_surface(8, 1.0, 1, one, &r1, &prm, nullptr, nullptr) != FLUID_ERR_ARG) return fail("NULL values accepted");
    if (fluid_spheres_surface(8, 1.0, 0, nullptr, nullptr, &prm, val.data(), nullptr) != FLUID_OK || val[0] != 2.5f) return fail("no items");
    std::puts("host sanitizer run (sdf trail): ok");
    return 0;
}
