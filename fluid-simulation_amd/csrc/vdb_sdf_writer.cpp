// .vdb writer for the liquid surface (include/fluid_hip.h, "liquid surface") and the dense form of its leaf list — host only, no
// GPU, no OpenVDB.  The stream, the zip framing, the file header and everything of a grid in front of its tree are vdb_format.h's,
// shared with vdb_writer.cpp, whose own code describes a tree with every leaf of [lo,hi]^3 present and background 0; the rules of
// a leaf list, the dense scatter and the walk of the merges are leaf_list.h's.
//
// One FloatGrid named "surface", class "level set", in OpenVDB's file format 224 (the serialisation vdb_writer.cpp's head comment
// cites: io/Archive.cc:939-971,1243-1328, tree/RootNode.h:2257-2288, tree/InternalNode.h:2175-2195, tree/LeafNode.h:1321-1324,
// 1444-1453, io/Compression.h:462-639).  What differs from the density grid:
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
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vdb_format.h"

namespace {

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

using Mid = std::map<int, std::vector<std::pair<int, int>>>;   // slot of a 128^3 node in its root child -> (slot of the leaf, index in the list)

}  // namespace

extern "C" {

int fluid_sdf_to_dense(const fluid_sdf_grid_t* g, float* values, uint8_t* active)
{
    if (!values) return FLUID_ERR_ARG;
    const int rc = check_list(g);
    if (rc) return rc;
    const size_t nc = (size_t)g->n * g->n * g->n;
    for (size_t i = 0; i < nc; ++i) values[i] = g->background;
    if (active) memset(active, 0, nc);
    scatter_leaves(g, [&](size_t l, int off, size_t c) {
        values[c] = g->values[512 * l + off];
        if (active) active[c] = bit(g->active + 8 * l, off) ? 1 : 0;
    });
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
    auto n_leaves_of = [&](int p) { return parts[p].n_leaves; };
    auto origin_of = [&](int p, long l) { return org_of(&parts[p], l); };
    int64_t count = 0;
    for (int pass = 0; pass < (count_only ? 1 : 2); ++pass) {
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        count = 0;
        merge_walk(n_parts, n_leaves_of, origin_of, [&](const Org& o, int n_in, const int32_t* part, const int32_t* leaf) {
            if (pass == 1) {   // (the first pass counts)
                float* acc = values + 512 * (size_t)count;
                uint64_t* am = active + 8 * (size_t)count;
                for (int t = 0; t < n_in; ++t) {
                    const float* v = parts[part[t]].values + 512 * (size_t)leaf[t];
                    const uint64_t* m = parts[part[t]].active + 8 * (size_t)leaf[t];
                    if (t == 0) {
                        memcpy(acc, v, 512 * sizeof(float));
                        memcpy(am, m, 8 * sizeof(uint64_t));
                    } else {
                        fold_leaf(acc, am, v, m, bg);
                    }
                }
                memcpy(origin + 3 * (size_t)count, &o, sizeof o);
            }
            count++;
            return true;
        });
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
    std::vector<float> acc(512), low(512), bd2(512), bval(512), bvel(1536);
    std::vector<uint32_t> bid(512);
    std::vector<uint8_t> has(512);
    uint64_t am[8];
    auto n_leaves_of = [&](int p) { return parts[p].n_leaves; };
    auto origin_of = [&](int p, long l) { return org_of(&parts[p], l); };
    int64_t count = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && (count_only || count == 0)) break;
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        count = 0;
        const bool merged = merge_walk(n_parts, n_leaves_of, origin_of, [&](const Org& o, int n_in, const int32_t* part, const int32_t* leaf) {
            if (pass == 0 && n_in == 1) {   // a leaf that one part alone lists cannot contradict itself: counted, not folded
                count++;
                return true;
            }
            std::fill(has.begin(), has.end(), 0);
            for (int t = 0; t < n_in; ++t) {
                const int p = part[t];
                const size_t l = (size_t)leaf[t];
                const float* v = parts[p].values + 512 * l;
                const uint64_t* m = parts[p].active + 8 * l;
                const uint32_t* pi = attrs[p].id + 512 * l;
                const float *pv = attrs[p].velocity + 1536 * l, *pd = attrs[p].dist2 + 512 * l;
                if (t == 0) {
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
                if (has[i] && !same_bits(low[i], bval[i])) return false;   // (pass 0 meets it first: nothing is written yet)
                if (!bit(am, i)) bid[i] = FLUID_SDF_NO_ID, bvel[i] = bvel[512 + i] = bvel[1024 + i] = 0.0f;
            }
            if (pass == 1) {
                memcpy(origin + 3 * (size_t)count, &o, sizeof o);
                memcpy(values + 512 * (size_t)count, acc.data(), 512 * sizeof(float));
                memcpy(active + 8 * (size_t)count, am, sizeof am);
                memcpy(id + 512 * (size_t)count, bid.data(), 512 * sizeof(uint32_t));
                memcpy(velocity + 1536 * (size_t)count, bvel.data(), 1536 * sizeof(float));
            }
            count++;
            return true;
        });
        if (!merged) return -FLUID_ERR_ARG;
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
    std::map<Org, Mid> roots;   // root children by origin, in Org's order (math/Coord.h:180-185)
    int32_t bmin[3] = {INT_MAX, INT_MAX, INT_MAX}, bmax[3] = {INT_MIN, INT_MIN, INT_MIN};
    int64_t voxels = 0, n_int1 = 0;
    for (size_t l = 0; l < nl; ++l) {
        const int32_t* o = g->origin + 3 * l;
        const float* v = g->values + 512 * l;
        const uint64_t* m = g->active + 8 * l;
        const int c = leaf_code(v, m, bg);
        if (c < 0) return FLUID_ERR_ARG;
        code[l] = (int8_t)c;
        const Org r{floor_to(o[0], INT2), floor_to(o[1], INT2), floor_to(o[2], INT2)};
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
    file_header(o, 1);
    // "class" and "name" beside the file_* statistics; a unique non-empty name is the descriptor's too
    std::vector<Meta> md = file_stats(comp, bmin, bmax, tree_mem_bytes((int64_t)roots.size(), n_int1, (int64_t)nl), voxels);
    md.insert(md.begin(), Meta{"class", "string", "level set"});
    md.push_back(Meta{"name", "string", "surface"});
    const size_t off = grid_head(o, "surface", comp, md, (double)(bg / g->half_width), bg, (uint32_t)roots.size());
    // ---- topology ----
    for (auto& r : roots) {
        const int32_t org[3] = {r.first.x, r.first.y, r.first.z};
        o.raw(org, sizeof(org));
        std::vector<uint64_t> cm(32 * 32 * 32 / 64, 0);
        for (auto& mid : r.second) cm[(size_t)mid.first >> 6] |= 1ull << (mid.first & 63);
        o.raw(cm.data(), cm.size() * 8);
        background_tiles(o, cm.size() * 8, comp);
        for (auto& mid : r.second) {
            uint64_t lm[64] = {};
            for (auto& lf : mid.second) lm[lf.first >> 6] |= 1ull << (lf.first & 63);
            o.raw(lm, sizeof(lm));
            background_tiles(o, sizeof(lm), comp);
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
