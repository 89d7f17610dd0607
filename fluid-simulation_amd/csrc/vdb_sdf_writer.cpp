// .vdb writer for the liquid surface (include/fluid_hip.h, "liquid surface") and the dense form of its leaf list — host only, no
// GPU, no OpenVDB.  It shares no code with vdb_writer.cpp, whose constants describe a tree with every leaf of [lo,hi]^3 present and
// background 0; the rules of a leaf list (check_list) are leaf_list.h's.
//
// One FloatGrid named "surface", class "level set", in OpenVDB's file format 224 (the serialisation vdb_writer.cpp restates:
// io/Archive.cc:939-971,1243-1328, tree/RootNode.h:2257-2288, tree/InternalNode.h:2175-2195, tree/LeafNode.h:1321-1324,1444-1453,
// io/Compression.h:462-639).  What differs from the density grid:
//   topology   only the listed leaves exist.  A root child (4096^3) and a 128^3 node exist where a listed leaf lies; every other
//              slot of an internal node is an inactive background tile, so its value mask is all off and writeCompressedValues
//              finds one inactive value equal to the background (child slots are skipped, Compression.h:506): metadata byte 0 and
//              an empty value array.  The root has no tiles.  A grid with no listed leaf has no root child.
//   leaves     value mask = the active mask; only the active values are stored (COMPRESS_ACTIVE_MASK).  The inactive ones are
//              coded by the metadata byte (Compression.h:519-562): 0 = none, or all +background; 1 = all -background; 3 = both,
//              followed by a selection mask whose on bits mark the inactive voxels that hold +background.
//   metadata   "class" = "level set" and "name" = "surface" beside the file_* statistics (bounding box and count of the ACTIVE
//              voxels; std::map order = by name).  A grid with a unique non-empty name keeps it in the descriptor
//              (io/Archive.cc:1203-1206).
//   transform  UniformScaleMap(voxel size), voxel size = background / half_width.
// Parity with the library is unpinned, as for the density files; tests/test_sdf_host.py re-reads the files with tests/vdb_reader.py.
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "leaf_list.h"

namespace {

struct Out {
    FILE* f = nullptr;
    size_t at = 0;
    bool ok = true;
    std::vector<char> buf;
    std::vector<unsigned char> zbuf;
    void flush()
    {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), f) != buf.size()) ok = false;
        buf.clear();
    }
    void raw(const void* p, size_t n)
    {
        const char* c = (const char*)p;
        if (n) buf.insert(buf.end(), c, c + n);
        at += n;
        if (buf.size() >= (size_t)1 << 20) flush();
    }
    template <typename T> void put(T v) { raw(&v, sizeof(T)); }
    void str(const std::string& s) { put<uint32_t>((uint32_t)s.size()); raw(s.data(), s.size()); }
    void zeros(size_t n) { const std::vector<char> z(n, 0); raw(z.data(), n); }
    void patch64(size_t where, int64_t v)
    {
        flush();
        if (fseeko(f, (off_t)where, SEEK_SET) != 0 || fwrite(&v, 1, 8, f) != 8 || fseeko(f, 0, SEEK_END) != 0) ok = false;
    }
    // writeData (io/Compression.h:253-264): zipToStream with COMPRESS_ZIP (io/Compression.cc:70-100), the raw bytes otherwise
    void data(const void* p, size_t n, uint32_t compression)
    {
        if (!(compression & 0x1)) { raw(p, n); return; }
        static const unsigned char none = 0;
        const Bytef* src = n ? (const Bytef*)p : &none;
        uLongf zn = compressBound((uLong)n);
        zbuf.resize(zn);
        const int st = compress2(zbuf.data(), &zn, src, (uLong)n, Z_DEFAULT_COMPRESSION);
        if (st == Z_OK && zn < n) {
            put<int64_t>((int64_t)zn);
            raw(zbuf.data(), zn);
        } else {
            put<int64_t>(-(int64_t)n);
            raw(p, n);
        }
    }
};

constexpr int INT1 = 128, INT2 = 4096;

template <typename T> void meta(Out& o, const char* name, const char* type, const T* v, uint32_t bytes)
{
    o.str(name); o.str(type); o.put<uint32_t>(bytes); o.raw(v, bytes);
}

inline bool bit(const uint64_t* m, int off) { return (m[off >> 6] >> (off & 63)) & 1; }
inline bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// the per-node metadata byte of a leaf, or -1: an inactive value that is neither +bg nor -bg
int leaf_code(const float* v, const uint64_t* m, float bg)
{
    bool neg = false, pos = false;
    for (int off = 0; off < 512; ++off) {
        if (bit(m, off)) continue;
        if (same_bits(v[off], bg)) pos = true;
        else if (same_bits(v[off], -bg)) neg = true;
        else return -1;
    }
    return !neg ? 0 : (!pos ? 1 : 3);   // NO_MASK_OR_INACTIVE_VALS, NO_MASK_AND_MINUS_BG, MASK_AND_NO_INACTIVE_VALS (io/Compression.h:94-100)
}

// one more part's record of a leaf folded into acc / am (the first part's record is copied instead)
void fold_leaf(float* acc, uint64_t* am, const float* v, const uint64_t* m, float bg)
{
    for (int i = 0; i < 512; ++i) {
        const bool a_in = bit(m, i), a_acc = bit(am, i);
        if (!a_acc && !same_bits(acc[i], bg)) continue;    // inactive -bg so far: it stays
        if (!a_in) {
            if (same_bits(v[i], bg)) continue;             // this part has nothing to say
            acc[i] = v[i];                                 // inactive -bg beats whatever was there
            am[i >> 6] &= ~(1ull << (i & 63));
        } else if (!a_acc || v[i] < acc[i]) {              // active: the smallest value, the first part's bits on a tie
            acc[i] = v[i];
            am[i >> 6] |= 1ull << (i & 63);
        }
    }
}

// what fluid_sdf_grids_merge refuses in its parts
bool parts_merge(const fluid_sdf_grid_t* parts, int32_t n_parts)
{
    const float bg = parts[0].background;
    for (int p = 0; p < n_parts; ++p) {
        const fluid_sdf_grid_t& g = parts[p];
        if (check_list(&g) != FLUID_OK || g.n != parts[0].n || !same_bits(g.background, bg) || !same_bits(g.radius, parts[0].radius) ||
            !same_bits(g.half_width, parts[0].half_width))
            return false;
        for (int l = 0; l < g.n_leaves; ++l)
            if (leaf_code(g.values + 512 * (size_t)l, g.active + 8 * (size_t)l, bg) < 0) return false;
    }
    return true;
}

inline bool org_before(const int32_t* a, const int32_t* b) { return a[0] != b[0] ? a[0] < b[0] : a[1] != b[1] ? a[1] < b[1] : a[2] < b[2]; }

using Mid = std::map<int, std::vector<std::pair<int, int>>>;   // slot of a 128^3 node in its root child -> (slot of the leaf, index in the list)
struct Key {
    int x, y, z;
    bool operator<(const Key& b) const { return x != b.x ? x < b.x : y != b.y ? y < b.y : z < b.z; }   // math/Coord.h:180-185
};

}  // namespace

extern "C" {

int fluid_sdf_to_dense(const fluid_sdf_grid_t* g, float* values, uint8_t* active)
{
    if (!values) return FLUID_ERR_ARG;
    const int rc = check_list(g);
    if (rc) return rc;
    const int n = g->n, lo = -(n / 2);
    const size_t nc = (size_t)n * n * n;
    for (size_t i = 0; i < nc; ++i) values[i] = g->background;
    if (active) memset(active, 0, nc);
    for (int l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        const float* v = g->values + 512 * (size_t)l;
        const uint64_t* m = g->active + 8 * (size_t)l;
        for (int x = 0; x < 8; ++x)
            for (int y = 0; y < 8; ++y)
                for (int z = 0; z < 8; ++z) {
                    const int ax = o[0] + x - lo, ay = o[1] + y - lo, az = o[2] + z - lo;
                    if (ax < 0 || ax >= n || ay < 0 || ay >= n || az < 0 || az >= n) continue;
                    const int off = (x * 8 + y) * 8 + z;
                    const size_t c = ((size_t)ax * n + ay) * n + az;
                    values[c] = v[off];
                    if (active) active[c] = bit(m, off) ? 1 : 0;
                }
    }
    return FLUID_OK;
}

// Host only ("liquid surface (decomposed runs)").  A k-way merge of ascending lists: the smallest origin at the parts' cursors
// is the next merged leaf, every part that lists it is folded in, in part order.  Per voxel the three states are ordered
// inactive -bg < active (by value) < inactive +bg: the state decides first, the float value only among active voxels (a plain
// minimum of the values with the masks ORed would leave a -bg voxel active).
int64_t fluid_sdf_grids_merge(const fluid_sdf_grid_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active)
{
    const bool count_only = !origin && !values && !active;
    if (!parts || n_parts < 1 || (!count_only && (!origin || !values || !active))) return -FLUID_ERR_ARG;
    if (!parts_merge(parts, n_parts)) return -FLUID_ERR_ARG;
    const float bg = parts[0].background;
    std::vector<int32_t> cur((size_t)n_parts);
    int64_t count = 0;
    for (int pass = 0; pass < (count_only ? 1 : 2); ++pass) {
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        std::fill(cur.begin(), cur.end(), 0);
        count = 0;
        for (;;) {
            const int32_t* o = nullptr;   // the smallest origin at the parts' cursors
            for (int p = 0; p < n_parts; ++p) {
                if (cur[p] >= parts[p].n_leaves) continue;
                const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                if (!o || org_before(c, o)) o = c;
            }
            if (!o) break;
            const int32_t o3[3] = {o[0], o[1], o[2]};
            float* acc = pass == 1 ? values + 512 * (size_t)count : nullptr;
            uint64_t* am = pass == 1 ? active + 8 * (size_t)count : nullptr;
            int n_in = 0;
            for (int p = 0; p < n_parts; ++p) {
                if (cur[p] >= parts[p].n_leaves) continue;
                const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                if (c[0] != o3[0] || c[1] != o3[1] || c[2] != o3[2]) continue;
                const float* v = parts[p].values + 512 * (size_t)cur[p];
                const uint64_t* m = parts[p].active + 8 * (size_t)cur[p];
                cur[p]++;
                if (pass == 0) continue;
                if (n_in++ == 0) {
                    memcpy(acc, v, 512 * sizeof(float));
                    memcpy(am, m, 8 * sizeof(uint64_t));
                    continue;
                }
                fold_leaf(acc, am, v, m, bg);
            }
            if (pass == 1) memcpy(origin + 3 * (size_t)count, o3, sizeof o3);
            count++;
        }
    }
    return count;
}

// Host only ("liquid surface, attributes (decomposed runs)").  The same k-way merge; the geometry of a leaf is folded by the same
// fold_leaf, and beside it every voxel keeps the part that holds it active with the smallest (dist2, id), the first such part.
// Both passes compute a leaf into buffers of one leaf: the first counts and, in the leaves that several parts list, looks for a
// voxel whose closest part does not hold the smallest active value (a refusal must write nothing); the second computes every leaf
// and copies it into the caller's arrays.
int64_t fluid_sdf_attr_grids_merge(const fluid_sdf_grid_t* parts, const fluid_sdf_attr_part_t* attrs, int32_t n_parts, int64_t cap_leaves,
                                   int32_t* origin, float* values, uint64_t* active, uint32_t* id, float* velocity)
{
    const bool count_only = !origin && !values && !active && !id && !velocity;
    if (!parts || !attrs || n_parts < 1 || (!count_only && (!origin || !values || !active || !id || !velocity))) return -FLUID_ERR_ARG;
    if (!parts_merge(parts, n_parts)) return -FLUID_ERR_ARG;
    const float bg = parts[0].background;
    for (int p = 0; p < n_parts; ++p) {
        const fluid_sdf_grid_t& g = parts[p];
        const fluid_sdf_attr_part_t& a = attrs[p];
        if (a.n_leaves != g.n_leaves || (g.n_leaves > 0 && (!a.id || !a.velocity || !a.dist2))) return -FLUID_ERR_ARG;
        for (size_t i = 0; i < 512 * (size_t)g.n_leaves; ++i)
            if (bit(g.active + 8 * (i >> 9), (int)(i & 511)) && (!std::isfinite(a.dist2[i]) || a.id[i] == FLUID_SDF_NO_ID)) return -FLUID_ERR_ARG;
    }
    std::vector<int32_t> cur((size_t)n_parts);
    std::vector<float> acc(512), low(512), bd2(512), bval(512), bvel(1536);
    std::vector<uint32_t> bid(512);
    std::vector<uint8_t> has(512);
    uint64_t am[8];
    int64_t count = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && (count_only || count == 0)) break;
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        std::fill(cur.begin(), cur.end(), 0);
        count = 0;
        for (;;) {
            const int32_t* o = nullptr;   // the smallest origin at the parts' cursors
            for (int p = 0; p < n_parts; ++p) {
                if (cur[p] >= parts[p].n_leaves) continue;
                const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                if (!o || org_before(c, o)) o = c;
            }
            if (!o) break;
            const int32_t o3[3] = {o[0], o[1], o[2]};
            if (pass == 0) {   // a leaf that one part alone lists cannot contradict itself: counted, not folded
                int lists = 0, who = -1;
                for (int p = 0; p < n_parts; ++p) {
                    if (cur[p] >= parts[p].n_leaves) continue;
                    const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                    if (c[0] == o3[0] && c[1] == o3[1] && c[2] == o3[2]) ++lists, who = p;
                }
                if (lists == 1) {
                    cur[who]++;
                    count++;
                    continue;
                }
            }
            std::fill(has.begin(), has.end(), 0);
            int n_in = 0;
            for (int p = 0; p < n_parts; ++p) {
                if (cur[p] >= parts[p].n_leaves) continue;
                const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                if (c[0] != o3[0] || c[1] != o3[1] || c[2] != o3[2]) continue;
                const size_t l = (size_t)cur[p]++;
                const float* v = parts[p].values + 512 * l;
                const uint64_t* m = parts[p].active + 8 * l;
                const uint32_t* pi = attrs[p].id + 512 * l;
                const float *pv = attrs[p].velocity + 1536 * l, *pd = attrs[p].dist2 + 512 * l;
                if (n_in++ == 0) {
                    memcpy(acc.data(), v, 512 * sizeof(float));
                    memcpy(am, m, sizeof am);
                } else {
                    fold_leaf(acc.data(), am, v, m, bg);
                }
                for (int i = 0; i < 512; ++i) {
                    if (!bit(m, i)) continue;
                    if (!has[i] || v[i] < low[i]) low[i] = v[i];   // the smallest active value, the first part's bits on a tie
                    if (!has[i] || pd[i] < bd2[i] || (pd[i] == bd2[i] && pi[i] < bid[i])) {
                        bd2[i] = pd[i], bid[i] = pi[i], bval[i] = v[i];
                        bvel[i] = pv[i], bvel[512 + i] = pv[512 + i], bvel[1024 + i] = pv[1024 + i];
                    }
                    has[i] = 1;
                }
            }
            for (int i = 0; i < 512; ++i) {
                if (has[i] && !same_bits(low[i], bval[i])) return -FLUID_ERR_ARG;   // (pass 0 meets it first: nothing is written yet)
                if (!bit(am, i)) bid[i] = FLUID_SDF_NO_ID, bvel[i] = bvel[512 + i] = bvel[1024 + i] = 0.0f;
            }
            if (pass == 1) {
                memcpy(origin + 3 * (size_t)count, o3, sizeof o3);
                memcpy(values + 512 * (size_t)count, acc.data(), 512 * sizeof(float));
                memcpy(active + 8 * (size_t)count, am, sizeof am);
                memcpy(id + 512 * (size_t)count, bid.data(), 512 * sizeof(uint32_t));
                memcpy(velocity + 1536 * (size_t)count, bvel.data(), 1536 * sizeof(float));
            }
            count++;
        }
    }
    return count;
}

int fluid_write_vdb_sdf(const char* path, const fluid_sdf_grid_t* g, int32_t compression)
{
    if (!path || (compression != FLUID_VDB_ACTIVE_MASK && compression != FLUID_VDB_ZIP_ACTIVE_MASK)) return FLUID_ERR_ARG;
    int rc = check_list(g);
    if (rc) return rc;
    const float bg = g->background;
    if (!(bg > 0.0f) || !(g->half_width > 0.0f)) return FLUID_ERR_ARG;
    const size_t nl = (size_t)g->n_leaves;
    // per leaf: metadata byte; the tree the list spans; statistics of the active voxels
    std::vector<int8_t> code(nl);
    std::map<Key, Mid> roots;
    int32_t bmin[3] = {INT_MAX, INT_MAX, INT_MAX}, bmax[3] = {INT_MIN, INT_MIN, INT_MIN};
    int64_t voxels = 0, n_int1 = 0;
    for (size_t l = 0; l < nl; ++l) {
        const int32_t* o = g->origin + 3 * l;
        const float* v = g->values + 512 * l;
        const uint64_t* m = g->active + 8 * l;
        const int c = leaf_code(v, m, bg);
        if (c < 0) return FLUID_ERR_ARG;
        code[l] = (int8_t)c;
        const Key r{floor_to(o[0], INT2), floor_to(o[1], INT2), floor_to(o[2], INT2)};
        const int a[3] = {(o[0] - r.x) / INT1, (o[1] - r.y) / INT1, (o[2] - r.z) / INT1};
        const int q[3] = {((o[0] - r.x) % INT1) / LEAF, ((o[1] - r.y) % INT1) / LEAF, ((o[2] - r.z) % INT1) / LEAF};
        roots[r][(a[0] << 10) + (a[1] << 5) + a[2]].push_back({(q[0] << 8) + (q[1] << 4) + q[2], (int)l});
        for (int off = 0; off < 512; ++off)
            if (bit(m, off)) {
                const int p[3] = {o[0] + (off >> 6), o[1] + ((off >> 3) & 7), o[2] + (off & 7)};
                for (int k = 0; k < 3; ++k) {
                    bmin[k] = p[k] < bmin[k] ? p[k] : bmin[k];
                    bmax[k] = p[k] > bmax[k] ? p[k] : bmax[k];
                }
                ++voxels;
            }
    }
    for (auto& r : roots) n_int1 += (int64_t)r.second.size();   // (the list ascends in (x, y, z): so do the leaves of every 128^3 node)

    Out o;
    o.f = fopen(path, "wb");
    if (!o.f) return FLUID_ERR_ARG;
    const uint32_t comp = (uint32_t)compression;
    // ---- header (io/Archive.cc:939-971) ----
    o.put<int64_t>(0x56444220);
    o.put<uint32_t>(224);
    o.put<uint32_t>(4); o.put<uint32_t>(0);
    o.put<char>(1);
    {
        std::mt19937 ran((unsigned)(std::random_device()() + (unsigned)std::time(nullptr)));
        char u[37];
        const uint32_t a = ran(), b = ran(), c = ran(), d = ran();
        snprintf(u, sizeof(u), "%08x-%04x-4%03x-%04x-%04x%08x", a, b >> 16, b & 0xfff, 0x8000 | (c >> 18), c & 0xffff, d);
        o.raw(u, 36);
    }
    o.put<uint32_t>(0);   // file-level metadata: empty map
    o.put<int32_t>(1);    // one grid
    // ---- descriptor ----
    o.str("surface");
    o.str("Tree_float_5_4_3");
    o.str("");
    const size_t off = o.at;
    o.put<int64_t>(0); o.put<int64_t>(0); o.put<int64_t>(0);
    o.patch64(off, (int64_t)o.at);
    o.put<uint32_t>(comp);
    // ---- grid metadata ----
    // memUsage as vdb_writer.cpp's tree_mem_bytes counts it, for the nodes this tree has
    const int64_t mem = (8 + 56 + 2 * 568) + 56 + (int64_t)roots.size() * (32768 * 8 + 4096 + 4096 + 12) + n_int1 * (4096 * 8 + 512 + 512 + 12) +
                        (int64_t)nl * (96 + 2048);
    const std::string cs = (comp & 0x1) ? "zip + active values" : "active values";
    const std::string cls = "level set", name = "surface";
    o.put<uint32_t>(7);
    meta(o, "class", "string", cls.data(), (uint32_t)cls.size());
    meta(o, "file_bbox_max", "vec3i", bmax, 12);
    meta(o, "file_bbox_min", "vec3i", bmin, 12);
    meta(o, "file_compression", "string", cs.data(), (uint32_t)cs.size());
    meta(o, "file_mem_bytes", "int64", &mem, 8);
    meta(o, "file_voxel_count", "int64", &voxels, 8);
    meta(o, "name", "string", name.data(), (uint32_t)name.size());
    // ---- transform: UniformScaleMap(dx) = scale, voxel size, 1/scale, 1/scale^2, 1/(2 scale) (math/Maps.h ScaleMap::write) ----
    o.str("UniformScaleMap");
    const double dx = (double)(bg / g->half_width);
    const double sc[3] = {dx, dx, dx}, inv[3] = {1 / dx, 1 / dx, 1 / dx}, inv2[3] = {1 / (dx * dx), 1 / (dx * dx), 1 / (dx * dx)},
                 invt[3] = {1 / (2 * dx), 1 / (2 * dx), 1 / (2 * dx)};
    o.raw(sc, 24); o.raw(sc, 24); o.raw(inv, 24); o.raw(inv2, 24); o.raw(invt, 24);
    // ---- topology ----
    o.put<int32_t>(1);    // buffer count
    o.put<float>(bg);
    o.put<uint32_t>(0);   // root tiles
    o.put<uint32_t>((uint32_t)roots.size());
    for (auto& r : roots) {
        const int32_t org[3] = {r.first.x, r.first.y, r.first.z};
        o.raw(org, sizeof(org));
        std::vector<uint64_t> cm(32 * 32 * 32 / 64, 0);
        for (auto& mid : r.second) cm[(size_t)mid.first >> 6] |= 1ull << (mid.first & 63);
        o.raw(cm.data(), cm.size() * 8);
        o.zeros(cm.size() * 8);      // value mask: no active tile
        o.put<int8_t>(0);            // every tile holds the background
        o.data(nullptr, 0, comp);    // no active value
        for (auto& mid : r.second) {
            uint64_t lm[64] = {};
            for (auto& lf : mid.second) lm[lf.first >> 6] |= 1ull << (lf.first & 63);
            o.raw(lm, sizeof(lm));
            o.zeros(sizeof(lm));
            o.put<int8_t>(0);
            o.data(nullptr, 0, comp);
            for (auto& lf : mid.second) o.raw(g->active + 8 * (size_t)lf.second, 64);
        }
    }
    o.patch64(off + 8, (int64_t)o.at);    // block position
    // ---- buffers, in the order of the topology ----
    for (auto& r : roots)
        for (auto& mid : r.second)
            for (auto& lf : mid.second) {
                const size_t l = (size_t)lf.second;
                const float* v = g->values + 512 * l;
                const uint64_t* m = g->active + 8 * l;
                o.raw(m, 64);
                o.put<int8_t>(code[l]);
                float act[512];
                int na = 0;
                uint64_t sel[8] = {};
                for (int k = 0; k < 512; ++k) {
                    if (bit(m, k)) act[na++] = v[k];
                    else if (same_bits(v[k], bg)) sel[k >> 6] |= 1ull << (k & 63);
                }
                if (code[l] == 3) o.raw(sel, sizeof(sel));
                o.data(act, (size_t)na * sizeof(float), comp);
            }
    o.patch64(off + 16, (int64_t)o.at);   // end position
    o.flush();
    const int frc = fclose(o.f);
    if (o.ok && frc == 0) return FLUID_OK;
    remove(path);   // a short write leaves no partial file behind
    return FLUID_ERR_ARG;   // (the ABI has no code of its own for I/O: an unwritable path is a bad argument, as in vdb_writer.cpp)
}

}  // extern "C"
