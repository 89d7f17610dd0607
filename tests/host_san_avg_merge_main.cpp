// fluid_sdf_avg_grids_merge under AddressSanitizer + UBSan (tests/test_sdf_avg_merge_host.py builds and runs this with g++ together
// with sdf_avg_host.cpp).  The rank records come from the test (tests/sdf_avg_part_ref.py record(), written to <dir>/san_parts_<i>.bin:
// an odd n whose first leaf starts outside the grid, an empty part, leaves that one, two and three parts list); the merged lists go
// to <dir>/san_merged_<i>.bin for the test to compare with the library's own bytes and with the reference.  Exact capacity, the
// count-only call, a capacity one too small and every refusal run here too, each on copies of exactly the size the call may read.
// File of parts: int32 n_parts, then per part int32 n, n_leaves, float background, radius, half_width, dx, influence,
// int32 origin[3 k], float dist2[512 k], uint64 sums[2048 k].  File of a merge: int64 k, int32 origin[3 k], float values[512 k],
// uint64 active[8 k].
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "fluid_hip.h"

static int fail(const char* what)
{
    std::fprintf(stderr, "FAILED: %s\n", what);
    return 1;
}

struct Part {
    fluid_sdf_avg_part_t c{};
    std::vector<int32_t> origin;
    std::vector<float> dist2;
    std::vector<uint64_t> sums;
    void point()
    {
        c.origin = origin.empty() ? nullptr : origin.data();
        c.dist2 = dist2.empty() ? nullptr : dist2.data();
        c.sums = sums.empty() ? nullptr : sums.data();
    }
};

static bool read_parts(const std::string& path, std::vector<Part>& parts)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    int32_t np = 0;
    bool ok = std::fread(&np, 4, 1, f) == 1 && np >= 0 && np < 64;
    parts.assign(ok ? (size_t)np : 0, Part{});
    for (Part& p : parts) {
        int32_t h[2];
        float s[5];
        ok = ok && std::fread(h, 4, 2, f) == 2 && std::fread(s, 4, 5, f) == 5 && h[1] >= 0 && h[1] < 100000;
        if (!ok) break;
        const size_t k = (size_t)h[1];
        p.c.n = h[0], p.c.n_leaves = h[1];
        p.c.background = s[0], p.c.radius = s[1], p.c.half_width = s[2], p.c.dx = s[3], p.c.influence = s[4];
        p.origin.resize(3 * k), p.dist2.resize(512 * k), p.sums.resize(2048 * k);
        ok = std::fread(p.origin.data(), 4, 3 * k, f) == 3 * k && std::fread(p.dist2.data(), 4, 512 * k, f) == 512 * k &&
             std::fread(p.sums.data(), 8, 2048 * k, f) == 2048 * k;
        p.point();
    }
    std::fclose(f);
    return ok;
}

static int64_t merge(const std::vector<Part>& parts, int64_t cap, int32_t* o, float* v, uint64_t* a)
{
    std::vector<fluid_sdf_avg_part_t> c;
    for (const Part& p : parts) c.push_back(p.c);
    return fluid_sdf_avg_grids_merge(c.data(), (int32_t)c.size(), cap, o, v, a);
}

// the call is refused and writes nothing into outputs that would hold the whole merge
static bool refused(const std::vector<Part>& parts, int64_t k)
{
    std::vector<int32_t> o(3 * (size_t)k + 3, 0x5a5a5a5a);
    std::vector<float> v(512 * (size_t)k + 512, -77.0f);
    std::vector<uint64_t> a(8 * (size_t)k + 8, 0x1234u);
    if (merge(parts, k, o.data(), v.data(), a.data()) != -FLUID_ERR_ARG) return false;
    if (merge(parts, 0, nullptr, nullptr, nullptr) != -FLUID_ERR_ARG) return false;
    for (int32_t x : o) if (x != 0x5a5a5a5a) return false;
    for (float x : v) if (x != -77.0f) return false;
    for (uint64_t x : a) if (x != 0x1234u) return false;
    return true;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int sets = argc > 2 ? std::atoi(argv[2]) : 0;
    if (sets < 1) return fail("usage: <dir> <number of part files>");
    for (int i = 0; i < sets; ++i) {
        std::vector<Part> parts;
        if (!read_parts(dir + "/san_parts_" + std::to_string(i) + ".bin", parts) || parts.empty()) return fail("read");
        const int64_t k = merge(parts, 0, nullptr, nullptr, nullptr);
        if (k < 0) return fail("count");
        std::vector<int32_t> o(3 * (size_t)k);        // exactly k leaves: one voxel too far is ASan's to find
        std::vector<float> v(512 * (size_t)k);
        std::vector<uint64_t> a(8 * (size_t)k);
        if (k > 0 && merge(parts, k, o.data(), v.data(), a.data()) != k) return fail("merge");
        if (k > 0 && merge(parts, k - 1, o.data(), v.data(), a.data()) != -FLUID_ERR_ARG) return fail("a capacity one too small accepted");
        if (k > 0 && (merge(parts, k, nullptr, v.data(), a.data()) != -FLUID_ERR_ARG || merge(parts, k, o.data(), nullptr, a.data()) != -FLUID_ERR_ARG ||
                      merge(parts, k, o.data(), v.data(), nullptr) != -FLUID_ERR_ARG))
            return fail("a missing output accepted");
        const std::string path = dir + "/san_merged_" + std::to_string(i) + ".bin";
        std::FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(&k, 8, 1, f) != 1 || std::fwrite(o.data(), 4, o.size(), f) != o.size() || std::fwrite(v.data(), 4, v.size(), f) != v.size() ||
            std::fwrite(a.data(), 8, a.size(), f) != a.size() || std::fclose(f) != 0)
            return fail("write");
        if (i > 0) continue;
        // ---- the refusals, on the first set (at least two parts, the first of them with leaves)
        if (parts.size() < 2 || parts[0].c.n_leaves < 2) return fail("the first set is too small for the refusals");
        if (fluid_sdf_avg_grids_merge(nullptr, 1, 0, nullptr, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("NULL parts accepted");
        if (fluid_sdf_avg_grids_merge(&parts[0].c, 0, 0, nullptr, nullptr, nullptr) != -FLUID_ERR_ARG) return fail("n_parts = 0 accepted");
        for (int s = 0; s < 6; ++s) {                   // a scalar that differs as a bit pattern
            std::vector<Part> q = parts;
            for (Part& p : q) p.point();
            fluid_sdf_avg_part_t& c = q[1].c;
            if (s == 0) c.n += 1;
            float* fl[] = {nullptr, &c.background, &c.radius, &c.half_width, &c.dx, &c.influence};
            if (s > 0) *fl[s] = std::nextafterf(*fl[s], 100.0f);
            if (!refused(q, k)) return fail("parts of different scalars accepted");
        }
        for (int s = 0; s < 9; ++s) {                   // a bad list, a missing array, a bad voxel
            std::vector<Part> q = parts;
            for (Part& p : q) p.point();
            Part& p = q[0];
            size_t in = 0;                              // a voxel of the first part that carries sums
            while (in < p.dist2.size() && !(p.dist2[in] > 0.0f && std::isfinite(p.dist2[in]))) ++in;
            if (in == p.dist2.size()) return fail("no voxel with sums in the first part");
            const size_t l = in / 512, off = in % 512;
            if (s == 0) std::swap(p.origin[0], p.origin[3]), std::swap(p.origin[1], p.origin[4]), std::swap(p.origin[2], p.origin[5]);   // descending
            if (s == 1) p.origin[2] += 4;               // off the 8-grid
            if (s == 2) p.origin[0] = 8 * 4096;         // outside the grid's leaves
            if (s == 3) p.c.sums = nullptr;
            if (s == 4) p.c.dist2 = nullptr;
            if (s == 5) p.dist2[in] = NAN;
            if (s == 6) p.dist2[in] = -p.dist2[in];
            if (s == 7) p.dist2[in] = 0.0f;             // +0 beside sums
            if (s == 8) p.dist2[in] = INFINITY;         // +inf beside sums
            if ((s == 7 || s == 8) && !(p.sums[2048 * l + off] | p.sums[2048 * l + 512 + off] | p.sums[2048 * l + 1024 + off] | p.sums[2048 * l + 1536 + off]))
                p.sums[2048 * l + off] = 1;
            if (!refused(q, k)) return fail("a bad part accepted");
        }
        {
            std::vector<Part> q = parts;
            for (Part& p : q) p.point();
            q[0].dist2[0] = -0.0f;
            for (int c = 0; c < 4; ++c) q[0].sums[512 * c] = 0;
            if (!refused(q, k)) return fail("-0 accepted");
        }
    }
    std::puts("host sanitizer run (sdf avg merge): ok");
    return 0;
}
