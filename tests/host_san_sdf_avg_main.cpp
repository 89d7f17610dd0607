// fluid_particles_surface under AddressSanitizer + UBSan (tests/test_sdf_avg_host.py builds and runs this with g++ together with
// sdf_avg_host.cpp): a filled block beside scattered particles, some outside the grid and one NaN, on n = 9 (odd: a partial last
// cell row) and n = 16, both kinds; 3000 particles in one cell for the large sums; the promises of the definition (never outside
// the spheres); refused arguments.  The averaged grids are written to <dir>/san_avg_<n>.bin for the test to compare with the
// library's own bytes.
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

// the same particles as tests/test_sdf_avg_host.py::san_particles makes (same generator, same order)
static std::vector<double> particles(int n)
{
    const int lo = -(n / 2), hi = lo + n - 1;
    uint32_t s = 2024u + (uint32_t)n;
    std::vector<double> p;
    for (int x = -2; x < 2; ++x)
        for (int y = -2; y < 2; ++y)
            for (int z = -2; z < 2; ++z)
                for (int k = 0; k < 4; ++k)
                    for (int c : {x, y, z}) p.push_back(c + uni(s, -0.5, 0.5));
    for (int i = 0; i < 60; ++i)
        for (int a = 0; a < 3; ++a) p.push_back(uni(s, lo - 1.0, hi + 1.0));
    p.insert(p.end(), {NAN, 0.0, 0.0});
    return p;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const fluid_sdf_params_t prm = {1.0, 3.0};
    const fluid_sdf_surface_t avg = {FLUID_SDF_SURFACE_AVERAGED, 0, 3.0}, sph = {FLUID_SDF_SURFACE_SPHERES, 0, 0.0};
    for (int n : {9, 16}) {
        const std::vector<double> p = particles(n);
        const int64_t np = (int64_t)(p.size() / 3);
        const size_t nc = (size_t)n * n * n;
        std::vector<float> va(nc), vs(nc), v0(nc);
        std::vector<uint8_t> aa(nc), as(nc);
        if (fluid_particles_surface(n, 1.0, np, p.data(), &prm, &avg, va.data(), aa.data()) != FLUID_OK) return fail("averaged");
        if (fluid_particles_surface(n, 1.0, np, p.data(), &prm, &sph, vs.data(), as.data()) != FLUID_OK) return fail("spheres");
        if (fluid_particles_surface(n, 1.0, np, p.data(), &prm, nullptr, v0.data(), nullptr) != FLUID_OK) return fail("spheres, no mask");
        if (std::memcmp(vs.data(), v0.data(), nc * 4) != 0) return fail("NULL is not the spheres");
        size_t active = 0, differ = 0;
        for (size_t c = 0; c < nc; ++c) {
            if (aa[c] && !as[c]) return fail("active outside the spheres' active set");
            if (aa[c] && va[c] < vs[c]) return fail("a value below the spheres'");
            if (!as[c] && std::memcmp(&va[c], &vs[c], 4) != 0) return fail("an inactive voxel of the spheres changed");
            active += aa[c], differ += std::memcmp(&va[c], &vs[c], 4) != 0;
        }
        if (!active || !differ) return fail("the averaged surface is empty or is the spheres'");
        const std::string path = dir + "/san_avg_" + std::to_string(n) + ".bin";
        std::FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(va.data(), 4, nc, f) != nc || std::fwrite(aa.data(), 1, nc, f) != nc || std::fclose(f) != 0) return fail("write");
    }
    {   // 3000 particles in one cell: the sums go far beyond 32 bits
        const int n = 8;
        uint32_t s = 7u;
        std::vector<double> p;
        for (int i = 0; i < 3000; ++i)
            for (int a = 0; a < 3; ++a) p.push_back(1.0 + uni(s, -0.5, 0.5));
        std::vector<float> v((size_t)n * n * n);
        std::vector<uint8_t> a(v.size());
        const fluid_sdf_surface_t h4 = {FLUID_SDF_SURFACE_AVERAGED, 0, 4.0};
        if (fluid_particles_surface(n, 0.5, 3000, p.data(), &prm, &h4, v.data(), a.data()) != FLUID_OK) return fail("one full cell");
        const size_t c = ((size_t)(1 + 4) * n + (1 + 4)) * n + (1 + 4);   // voxel (1, 1, 1): the average is close to it
        if (!a[c] || !(v[c] < -0.45f)) return fail("one full cell: the centre");
    }
    std::vector<float> v(512);
    const double one[3] = {0.0, 0.0, 0.0};
    const fluid_sdf_surface_t bad[] = {{2, 0, 3.0}, {-1, 0, 3.0}, {1, 1, 3.0}, {1, 0, 0.0}, {1, 0, -1.0}, {1, 0, 4.5}, {1, 0, NAN}};
    for (const fluid_sdf_surface_t& b : bad)
        if (fluid_particles_surface(8, 1.0, 1, one, &prm, &b, v.data(), nullptr) != FLUID_ERR_ARG) return fail("a bad surface accepted");
    const fluid_sdf_params_t wide = {2.0, 2.5};
    if (fluid_particles_surface(8, 1.0, 1, one, &wide, &avg, v.data(), nullptr) != FLUID_ERR_ARG) return fail("R + w > 4 accepted");
    if (fluid_particles_surface(0, 1.0, 1, one, &prm, &avg, v.data(), nullptr) != FLUID_ERR_ARG) return fail("n = 0 accepted");
    if (fluid_particles_surface(8, 0.0, 1, one, &prm, &avg, v.data(), nullptr) != FLUID_ERR_ARG) return fail("dx = 0 accepted");
    if (fluid_particles_surface(8, 1.0, 1, nullptr, &prm, &avg, v.data(), nullptr) != FLUID_ERR_ARG) return fail("NULL positions accepted");
    if (fluid_particles_surface(8, 1.0, 1, one, nullptr, &avg, v.data(), nullptr) != FLUID_ERR_ARG) return fail("NULL parameters accepted");
    if (fluid_particles_surface(8, 1.0, 1, one, &prm, &avg, nullptr, nullptr) != FLUID_ERR_ARG) return fail("NULL values accepted");
    if (fluid_particles_surface(8, 1.0, 0, nullptr, &prm, &avg, v.data(), nullptr) != FLUID_OK || v[0] != 3.0f) return fail("no particles");
    std::puts("host sanitizer run (sdf avg): ok");
    return 0;
}
