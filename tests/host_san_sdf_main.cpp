// The liquid-surface half of the host code under AddressSanitizer + UBSan (tests/test_sdf_host.py builds and runs this with g++
// together with vdb_sdf_writer.cpp): leaf lists made here — every kind of leaf, partial edge leaves, enough leaves for several
// 128^3 nodes and root children — through fluid_sdf_to_dense and fluid_write_vdb_sdf (both compressions); refused lists.
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

struct List {
    std::vector<int32_t> origin;
    std::vector<float> values;
    std::vector<uint64_t> active;
    fluid_sdf_grid_t g;
    void bind(int n, float bg)
    {
        g.n = n;
        g.n_leaves = (int32_t)(origin.size() / 3);
        g.background = bg, g.radius = 1.5f, g.half_width = 2.5f;
        g.origin = origin.data(), g.values = values.data(), g.active = active.data();
    }
};

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// every `every`-th leaf of the grid, kinds in turn: mixed with both inactive signs / all -bg / all active / active and +bg
static void make(int n, int every, float bg, List& L)
{
    const int lo = -(n / 2), hi = lo + n - 1, l0 = lo & ~7, l1 = hi & ~7;
    uint32_t s = 12345u + (uint32_t)n;
    int count = 0;
    for (int ox = l0; ox <= l1; ox += 8)
        for (int oy = l0; oy <= l1; oy += 8)
            for (int oz = l0; oz <= l1; oz += 8) {
                const bool corner = (ox == l0 || ox == l1) && (oy == l0 || oy == l1) && (oz == l0 || oz == l1);
                if (count++ % every != 0 && !corner) continue;
                const int kind = count % 4;
                float v[512];
                uint64_t m[8] = {};
                for (int off = 0; off < 512; ++off) {
                    const int x = ox + (off >> 6), y = oy + ((off >> 3) & 7), z = oz + (off & 7);
                    const bool in = x >= lo && x <= hi && y >= lo && y <= hi && z >= lo && z <= hi;
                    const uint32_t r = rnd(s) >> 8;
                    v[off] = bg;
                    if (!in) continue;
                    const float d = bg * ((float)(r & 0xffff) / 32768.f - 1.f);
                    bool on = false;
                    if (kind == 0) { on = r % 5 > 1; if (!on) v[off] = (r % 5 == 0) ? -bg : bg; }
                    else if (kind == 1) v[off] = -bg;
                    else if (kind == 2) on = true;
                    else on = (r & 1) != 0;
                    if (on) { v[off] = d; m[off >> 6] |= 1ull << (off & 63); }
                }
                L.origin.insert(L.origin.end(), {ox, oy, oz});
                L.values.insert(L.values.end(), v, v + 512);
                L.active.insert(L.active.end(), m, m + 8);
            }
    L.bind(n, bg);
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const float bg = 2.5f;
    for (int n : {8, 25, 40, 130}) {
        List L;
        make(n, n == 130 ? 97 : 1, bg, L);
        if (L.g.n_leaves < 1) return fail("list");
        const size_t nc = (size_t)n * n * n;
        const int lo = -(n / 2);
        std::vector<float> dv(nc, 7.f);
        std::vector<uint8_t> da(nc, 9);
        if (fluid_sdf_to_dense(&L.g, dv.data(), da.data()) != FLUID_OK) return fail("to_dense");
        std::vector<float> dv2(nc, 7.f);
        if (fluid_sdf_to_dense(&L.g, dv2.data(), nullptr) != FLUID_OK || std::memcmp(dv.data(), dv2.data(), nc * 4) != 0) return fail("to_dense without a mask");
        std::vector<char> seen(nc, 0);
        for (int l = 0; l < L.g.n_leaves; ++l)
            for (int off = 0; off < 512; ++off) {
                const int ax = L.origin[3 * l] + (off >> 6) - lo, ay = L.origin[3 * l + 1] + ((off >> 3) & 7) - lo, az = L.origin[3 * l + 2] + (off & 7) - lo;
                if (ax < 0 || ax >= n || ay < 0 || ay >= n || az < 0 || az >= n) continue;
                const size_t c = ((size_t)ax * n + ay) * n + az;
                seen[c] = 1;
                const bool on = (L.active[8 * (size_t)l + (off >> 6)] >> (off & 63)) & 1;
                if (std::memcmp(&dv[c], &L.values[512 * (size_t)l + off], 4) != 0 || da[c] != (on ? 1 : 0)) return fail("to_dense: a listed voxel");
            }
        for (size_t c = 0; c < nc; ++c)
            if (!seen[c] && (dv[c] != bg || da[c] != 0)) return fail("to_dense: an unlisted voxel");
        const std::string z = dir + (n == 40 ? "/san_zip.vdb" : "/san_z.vdb"), a = dir + "/san_mask.vdb";
        if (fluid_write_vdb_sdf(z.c_str(), &L.g, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_OK) return fail("write (zip)");
        if (fluid_write_vdb_sdf(a.c_str(), &L.g, FLUID_VDB_ACTIVE_MASK) != FLUID_OK) return fail("write (active mask)");
        // refused lists: nothing is read beyond the list, no file is made
        const std::string bad = dir + "/san_bad.vdb";
        List B = L;
        B.bind(n, bg);
        B.origin[2] += 4;
        if (fluid_sdf_to_dense(&B.g, dv.data(), da.data()) != FLUID_ERR_ARG) return fail("unaligned origin accepted");
        if (fluid_write_vdb_sdf(bad.c_str(), &B.g, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_ERR_ARG) return fail("unaligned origin written");
        B.origin = L.origin;
        B.origin[0] = (lo & ~7) - 8;
        if (fluid_write_vdb_sdf(bad.c_str(), &B.g, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_ERR_ARG) return fail("outside origin accepted");
        if (L.g.n_leaves > 1) {
            B.origin = L.origin;
            for (int k = 0; k < 3; ++k) B.origin[3 + k] = B.origin[k];
            if (fluid_sdf_to_dense(&B.g, dv.data(), nullptr) != FLUID_ERR_ARG) return fail("duplicate origin accepted");
        }
        fluid_sdf_grid_t nul = L.g;
        nul.active = nullptr;
        if (fluid_sdf_to_dense(&nul, dv.data(), nullptr) != FLUID_ERR_ARG) return fail("null mask array accepted");
        if (std::FILE* f = std::fopen(bad.c_str(), "rb")) { std::fclose(f); return fail("a refused list left a file"); }
        fluid_sdf_grid_t empty = {n, 0, bg, 1.5f, 2.5f, nullptr, nullptr, nullptr};
        if (fluid_sdf_to_dense(&empty, dv.data(), da.data()) != FLUID_OK) return fail("empty list refused");
        for (size_t c = 0; c < nc; ++c)
            if (dv[c] != bg || da[c] != 0) return fail("empty list: a voxel");
        if (fluid_write_vdb_sdf(a.c_str(), &empty, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_OK) return fail("empty list not written");
    }
    std::puts("host sanitizer run (sdf): ok");
    return 0;
}
