// The leaf path of the .vdb writer under AddressSanitizer + UBSan (tests/test_vdb_leaves.py builds and runs this with g++):
// leaf lists made here from dense arrays, written through fluid_write_vdb_leaves / fluid_vdb_append_leaves (one and two
// writers, both compressions, partial edge leaves, two 128^3 nodes per axis, enough leaves for the threaded share) and
// compared byte for byte, outside the uuid, with the dense path's files; fluid_leaves_to_dense; refused lists.
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
    L.g.origin = L.origin.data();
    L.g.values = L.values.data();
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
    for (int n : {8, 21, 40, 130}) {
        const size_t nc = (size_t)n * n * n;
        std::vector<float> sparse(nc, 0.f), full(nc);
        for (size_t i = 0; i < nc; ++i) full[i] = (i % 7 == 0) ? 0.f : (float)(i % 13) * 0.25f;   // every leaf listed
        sparse[0] = 1.5f;
        sparse[nc - 1] = -0.0f;
        for (size_t i = nc / 3; i < nc / 3 + (size_t)n; ++i) sparse[i] = (float)(i % 5);
        for (int comp : {FLUID_VDB_ZIP_ACTIVE_MASK, FLUID_VDB_ACTIVE_MASK}) {
            if (n == 130 && comp == FLUID_VDB_ZIP_ACTIVE_MASK) continue;   // (the sparse one below covers two nodes per axis with ZIP)
            Leaves L;
            make_leaves(n, full, L);
            const std::string a = dir + "/sl_dense.vdb", b = dir + "/sl_leaves.vdb";
            const float* gp[1] = {full.data()};
            if (fluid_write_vdb_ex(a.c_str(), n, 1, gp, comp) != FLUID_OK) return fail("dense write");
            if (fluid_write_vdb_leaves(b.c_str(), &L.g, comp) != FLUID_OK) return fail("leaf write");
            if (!same_file(a, b)) return fail("full grid: files differ");
            std::vector<float> back(nc, 7.f);
            if (fluid_leaves_to_dense(&L.g, back.data()) != FLUID_OK) return fail("leaves_to_dense");
            if (std::memcmp(back.data(), full.data(), nc * 4) != 0) return fail("leaves_to_dense values");
        }
        {   // one call on two writers that stand at different grids, against two dense appends
            Leaves L;
            make_leaves(n, sparse, L);
            if (L.g.n_leaves < 2) return fail("sparse list");
            const std::string d1 = dir + "/sl_d1.vdb", d2 = dir + "/sl_d2.vdb", l1 = dir + "/sl_l1.vdb", l2 = dir + "/sl_l2.vdb";
            const float* two[2] = {full.data(), sparse.data()};
            const float* one[1] = {sparse.data()};
            if (fluid_write_vdb(d1.c_str(), n, 2, two) != FLUID_OK || fluid_write_vdb(d2.c_str(), n, 1, one) != FLUID_OK) return fail("dense pair");
            fluid_vdb_writer_t* w[2] = {nullptr, nullptr};
            if (fluid_vdb_open(l1.c_str(), n, 2, FLUID_VDB_ZIP_ACTIVE_MASK, &w[0]) != FLUID_OK) return fail("open 1");
            if (fluid_vdb_open(l2.c_str(), n, 1, FLUID_VDB_ZIP_ACTIVE_MASK, &w[1]) != FLUID_OK) return fail("open 2");
            if (fluid_vdb_append(w[0], full.data()) != FLUID_OK) return fail("dense append");
            if (fluid_vdb_append_leaves(w, 2, &L.g) != FLUID_OK) return fail("append_leaves on two writers");
            if (fluid_vdb_append_leaves(w, 2, &L.g) != FLUID_ERR_STATE) return fail("full writers accepted a grid");
            fluid_vdb_writer_t* twice[2] = {w[0], w[0]};
            if (fluid_vdb_append_leaves(twice, 2, &L.g) != FLUID_ERR_ARG) return fail("one writer twice accepted");
            if (fluid_vdb_close(w[0]) != FLUID_OK || fluid_vdb_close(w[1]) != FLUID_OK) return fail("close");
            if (!same_file(d1, l1) || !same_file(d2, l2)) return fail("two writers: files differ");
            // refused lists: nothing is read beyond the list
            Leaves B = L;
            B.g.origin = B.origin.data(), B.g.values = B.values.data();
            B.origin[2] += 4;
            std::vector<float> back(nc);
            if (fluid_leaves_to_dense(&B.g, back.data()) != FLUID_ERR_ARG) return fail("off-grid origin accepted");
            B.origin = L.origin;
            B.origin[0] = (-(n / 2) & ~7) - 8;
            if (fluid_write_vdb_leaves(l1.c_str(), &B.g, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_ERR_ARG) return fail("outside origin accepted");
            B.origin = L.origin;
            for (int a = 0; a < 3; ++a) B.origin[3 + a] = B.origin[a];
            if (fluid_leaves_to_dense(&B.g, back.data()) != FLUID_ERR_ARG) return fail("duplicate origin accepted");
            fluid_leaf_grid_t empty = {n, 0, nullptr, nullptr};
            if (fluid_leaves_to_dense(&empty, back.data()) != FLUID_OK) return fail("empty list refused");
            for (float f : back)
                if (f != 0.f) return fail("empty list: non-zero value");
            if (fluid_write_vdb_leaves(l2.c_str(), &empty, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_OK) return fail("empty list not written");
            fluid_leaf_grid_t nul = {n, 1, nullptr, nullptr};
            if (fluid_leaves_to_dense(&nul, back.data()) != FLUID_ERR_ARG) return fail("null arrays accepted");
        }
    }
    std::puts("host sanitizer run (leaves): ok");
    return 0;
}
