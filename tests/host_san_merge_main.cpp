// fluid_leaf_grids_merge under AddressSanitizer + UBSan (tests/test_leaf_merge.py builds and runs this with g++): leaf lists of
// the blocks of a dense array (everything outside a block zeroed, cuts at multiples of 4 so that leaves are split), merged with
// exactly-sized output buffers and compared with the list of the whole array; the count-only call; every refused case with
// buffers that must stay untouched; the merged list written as a .vdb against the dense write.
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

struct Leaves {
    std::vector<int32_t> origin;
    std::vector<float> values;
    fluid_leaf_grid_t g;
};

// the leaves of `dense` with a non-zero bit pattern, ascending (x, y, z)
static void make_leaves(int n, const std::vector<float>& dense, Leaves& L)
{
    const int lo = -(n / 2), hi = lo + n - 1, l0 = lo & ~7, l1 = hi & ~7;
    L.origin.clear();
    L.values.clear();
    for (int ox = l0; ox <= l1; ox += 8)
        for (int oy = l0; oy <= l1; oy += 8)
            for (int oz = l0; oz <= l1; oz += 8) {
                float v[512] = {};
                bool any = false;
                for (int x = 0; x < 8; ++x)
                    for (int y = 0; y < 8; ++y)
                        for (int z = 0; z < 8; ++z) {
                            const int ax = ox + x - lo, ay = oy + y - lo, az = oz + z - lo;
                            if (ax < 0 || ax >= n || ay < 0 || ay >= n || az < 0 || az >= n) continue;
                            const float f = dense[((size_t)ax * n + ay) * n + az];
                            uint32_t bits;
                            std::memcpy(&bits, &f, 4);
                            any = any || bits != 0;
                            v[(x * 8 + y) * 8 + z] = f;
                        }
                if (!any) continue;
                L.origin.insert(L.origin.end(), {ox, oy, oz});
                L.values.insert(L.values.end(), v, v + 512);
            }
    L.g.n = n;
    L.g.n_leaves = (int32_t)(L.origin.size() / 3);
    L.g.origin = L.origin.empty() ? nullptr : L.origin.data();
    L.g.values = L.values.empty() ? nullptr : L.values.data();
}

static bool same_file(const std::string& a, const std::string& b)
{
    auto slurp = [](const std::string& p, std::vector<char>& out) {
        FILE* f = std::fopen(p.c_str(), "rb");
        if (!f) return false;
        char buf[65536];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
        std::fclose(f);
        return true;
    };
    std::vector<char> x, y;
    if (!slurp(a, x) || !slurp(b, y) || x.size() != y.size() || x.size() < 57) return false;
    std::memset(x.data() + 21, 0, 36);
    std::memset(y.data() + 21, 0, 36);
    return std::memcmp(x.data(), y.data(), x.size()) == 0;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    for (int n : {8, 33, 50}) {
        const size_t nc = (size_t)n * n * n;
        std::vector<float> dense(nc, 0.f);
        for (size_t i = 0; i < nc; ++i)
            if (i % 11 == 0 || (i / 97) % 5 == 0) dense[i] = (float)(i % 17) * 0.5f - 2.f;
        dense[nc / 2] = -0.0f;
        Leaves whole;
        make_leaves(n, dense, whole);
        // 2 x 2 x 2 blocks cut at c per axis (one block per axis when n is too small to cut)
        const int c = n >= 16 ? ((n / 2 + 2) & ~3) : n;
        std::vector<Leaves> parts;
        for (int bx = 0; bx < (c < n ? 2 : 1); ++bx)
            for (int by = 0; by < (c < n ? 2 : 1); ++by)
                for (int bz = 0; bz < (c < n ? 2 : 1); ++bz) {
                    std::vector<float> blk(nc, 0.f);
                    const int b[3] = {bx, by, bz};
                    int lo3[3], hi3[3];
                    for (int a = 0; a < 3; ++a) lo3[a] = b[a] ? c : 0, hi3[a] = b[a] ? n : c;
                    for (int x = lo3[0]; x < hi3[0]; ++x)
                        for (int y = lo3[1]; y < hi3[1]; ++y)
                            std::memcpy(&blk[((size_t)x * n + y) * n + lo3[2]], &dense[((size_t)x * n + y) * n + lo3[2]], (size_t)(hi3[2] - lo3[2]) * 4);
                    parts.emplace_back();
                    make_leaves(n, blk, parts.back());
                }
        std::vector<fluid_leaf_grid_t> gs;
        for (auto& p : parts) {
            p.g.origin = p.origin.empty() ? nullptr : p.origin.data();   // (the vector of parts moved its elements)
            p.g.values = p.values.empty() ? nullptr : p.values.data();
            gs.push_back(p.g);
        }
        gs.push_back(fluid_leaf_grid_t{n, 0, nullptr, nullptr});         // an empty part among full ones
        const int np = (int)gs.size();
        const int64_t k = fluid_leaf_grids_merge(gs.data(), np, 0, nullptr, nullptr);
        if (k != whole.g.n_leaves) return fail("count-only call");
        std::vector<int32_t> org(3 * (size_t)k);   // exactly sized: one element too many written is a sanitizer report
        std::vector<float> val(512 * (size_t)k);
        if (fluid_leaf_grids_merge(gs.data(), np, k, org.data(), val.data()) != k) return fail("merge");
        if (org != whole.origin || std::memcmp(val.data(), whole.values.data(), val.size() * 4) != 0) return fail("merged list differs from the whole grid's");
        // refused: buffers untouched
        std::vector<int32_t> org0(org.size(), 0x5a5a5a5a);
        std::vector<float> val0(val.size(), 7.f);
        auto untouched = [&] {
            for (int32_t o : org0) if (o != 0x5a5a5a5a) return false;
            for (float f : val0) if (f != 7.f) return false;
            return true;
        };
        if (k > 0 && fluid_leaf_grids_merge(gs.data(), np, k - 1, org0.data(), val0.data()) != -FLUID_ERR_ARG) return fail("short buffer accepted");
        std::vector<fluid_leaf_grid_t> bad = gs;
        bad.back().n = n + 1;
        if (fluid_leaf_grids_merge(bad.data(), np, k, org0.data(), val0.data()) != -FLUID_ERR_ARG) return fail("different n accepted");
        bad = gs;
        bad.push_back(gs[0]);                                            // the first block twice: its voxels are claimed twice
        if (gs[0].n_leaves > 0 && fluid_leaf_grids_merge(bad.data(), np + 1, k, org0.data(), val0.data()) != -FLUID_ERR_ARG) return fail("a voxel held twice accepted");
        if (gs[0].n_leaves > 1) {
            std::vector<int32_t> rev(gs[0].origin, gs[0].origin + 3 * (size_t)gs[0].n_leaves);
            for (int a = 0; a < 3; ++a) std::swap(rev[a], rev[3 + a]);
            bad = gs;
            bad[0].origin = rev.data();
            if (fluid_leaf_grids_merge(bad.data(), np, k, org0.data(), val0.data()) != -FLUID_ERR_ARG) return fail("descending part accepted");
        }
        if (fluid_leaf_grids_merge(gs.data(), 0, k, org0.data(), val0.data()) != -FLUID_ERR_ARG) return fail("no parts accepted");
        if (!untouched()) return fail("a refused merge wrote to the buffers");
        // all parts empty
        fluid_leaf_grid_t none[2] = {{n, 0, nullptr, nullptr}, {n, 0, nullptr, nullptr}};
        if (fluid_leaf_grids_merge(none, 2, 0, org0.data(), val0.data()) != 0 || !untouched()) return fail("empty parts");
        // the file of the merged list is the dense file
        const fluid_leaf_grid_t m = {n, (int32_t)k, org.data(), val.data()};
        const std::string a = dir + "/sm_dense.vdb", b = dir + "/sm_merged.vdb";
        const float* gp[1] = {dense.data()};
        if (fluid_write_vdb(a.c_str(), n, 1, gp) != FLUID_OK || fluid_write_vdb_leaves(b.c_str(), &m, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_OK) return fail("writes");
        if (!same_file(a, b)) return fail("merged file differs from the dense file");
    }
    std::puts("host sanitizer run (merge): ok");
    return 0;
}
