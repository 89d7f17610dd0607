// What the host code shares about a list of 8^3 leaves, ascending in (x, y, z) origin: the density list (fluid_leaf_grid_t:
// vdb_writer.cpp) and the level-set list (fluid_sdf_grid_t: vdb_sdf_writer.cpp, sdf_filter_host.cpp, mesh_host.cpp,
// render_host.cpp).  For both: the origin ordering, the list rules, the scatter into a dense array and the cursor walk of a merge
// of several lists.  For the level set: the search in a list, and the leaves and the 9^3 tiles the surface nets work on (what
// happens in a tile's cell is mesh_def.h's).  vdb_format.h includes it for the two writers.  Header only: every file that
// includes it compiles on its own.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "fluid_hip.h"

namespace {

constexpr int LEAF = 8;
inline int floor_to(int v, int m) { return v & ~(m - 1); }

struct Org {
    int32_t x, y, z;
    bool operator<(const Org& b) const { return x != b.x ? x < b.x : y != b.y ? y < b.y : z < b.z; }
    bool operator==(const Org& b) const { return x == b.x && y == b.y && z == b.z; }
};
template <typename Grid> inline Org org_of(const Grid* g, long l)
{
    const int32_t* p = g->origin + 3 * (size_t)l;
    return Org{p[0], p[1], p[2]};
}

// The list rules, for both kinds of list.  FLUID_OK, or FLUID_ERR_ARG: no arrays behind a non-empty list, an origin off the
// 8-grid, outside the leaves of [lo,hi]^3, or not strictly ascending in (x, y, z)
template <typename Grid> inline int check_origins(const Grid* g, bool arrays)
{
    if (!g || g->n < 1 || g->n > 4096 || g->n_leaves < 0) return FLUID_ERR_ARG;
    if (g->n_leaves > 0 && !arrays) return FLUID_ERR_ARG;
    const int lo = -(g->n / 2), hi = lo + g->n - 1, L0 = floor_to(lo, LEAF), L1 = floor_to(hi, LEAF);
    for (int i = 0; i < g->n_leaves; ++i) {
        const int32_t* o = g->origin + 3 * (size_t)i;
        for (int a = 0; a < 3; ++a)
            if ((o[a] & (LEAF - 1)) != 0 || o[a] < L0 || o[a] > L1) return FLUID_ERR_ARG;
        if (i > 0 && !(org_of(g, i - 1) < org_of(g, i))) return FLUID_ERR_ARG;
    }
    return FLUID_OK;
}
inline int check_list(const fluid_leaf_grid_t* g) { return check_origins(g, g && g->origin && g->values); }
inline int check_list(const fluid_sdf_grid_t* g) { return check_origins(g, g && g->origin && g->values && g->active); }

// The in-grid voxels of every leaf of a (checked) list: put(l, off, c), l = the leaf's index in the list, off = the voxel's offset
// in that leaf, c = its place in a dense [n^3] array, z fastest.
template <typename Grid, typename Put> inline void scatter_leaves(const Grid* g, Put put)
{
    const int n = g->n, lo = -(n / 2);
    for (int l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        for (int x = 0; x < 8; ++x)
            for (int y = 0; y < 8; ++y)
                for (int z = 0; z < 8; ++z) {
                    const int ax = o[0] + x - lo, ay = o[1] + y - lo, az = o[2] + z - lo;
                    if (ax < 0 || ax >= n || ay < 0 || ay >= n || az < 0 || az >= n) continue;
                    put((size_t)l, (x * 8 + y) * 8 + z, ((size_t)ax * n + ay) * n + az);
                }
    }
}

// The cursor walk of a k-way merge of (checked, so ascending) lists: the smallest origin at the parts' cursors is the next merged
// leaf.  n_leaves_of(p) and origin_of(p, l) describe part p; visit(origin, n_in, part, leaf) is called once per merged leaf, in
// ascending order, with the n_in >= 1 parts that list it, in part order, and the leaf's index in each.  False from visit ends
// the walk, which then returns false.
template <typename NLeavesOf, typename OriginOf, typename Visit>
inline bool merge_walk(int n_parts, NLeavesOf n_leaves_of, OriginOf origin_of, Visit visit)
{
    std::vector<int32_t> scratch(3 * (size_t)n_parts, 0);   // one allocation per walk: cursors, then what a visit is handed
    int32_t *cur = scratch.data(), *part = cur + n_parts, *leaf = part + n_parts;
    for (;;) {
        Org o{};
        bool any = false;
        for (int p = 0; p < n_parts; ++p) {
            if (cur[p] >= n_leaves_of(p)) continue;
            const Org c = origin_of(p, cur[p]);
            if (!any || c < o) o = c, any = true;
        }
        if (!any) return true;
        int n_in = 0;
        for (int p = 0; p < n_parts; ++p)
            if (cur[p] < n_leaves_of(p) && origin_of(p, cur[p]) == o) part[n_in] = p, leaf[n_in++] = cur[p]++;
        if (!visit(o, n_in, part, leaf)) return false;
    }
}

// index of the leaf at o in the (checked) list, or -1: bisection
inline long find_leaf(const fluid_sdf_grid_t* g, const Org& o)
{
    long a = 0, b = g->n_leaves;
    while (a < b) {
        const long m = (a + b) / 2;
        if (org_of(g, m) < o) a = m + 1;
        else b = m;
    }
    return a < g->n_leaves && org_of(g, a) == o ? a : -1;
}

// The leaves the surface nets work on, ascending.  A mixed cell has an inside corner, which lies in a listed leaf; its min corner
// lies in that leaf or in one of the seven leaves at -1: the listed leaves and those neighbours, where the grid has them.
inline std::vector<Org> mesh_work_list(const fluid_sdf_grid_t* g)
{
    const int L0 = floor_to(-(g->n / 2), LEAF);
    std::vector<Org> work;
    work.reserve((size_t)g->n_leaves * 2);
    for (long l = 0; l < g->n_leaves; ++l) {
        const Org o = org_of(g, l);
        for (int d = 0; d < 8; ++d) {
            const Org c{o.x - 8 * (d >> 2), o.y - 8 * ((d >> 1) & 1), o.z - 8 * (d & 1)};
            if (c.x >= L0 && c.y >= L0 && c.z >= L0) work.push_back(c);
        }
    }
    std::sort(work.begin(), work.end());
    work.erase(std::unique(work.begin(), work.end()), work.end());
    return work;
}

// The 9^3 tile of a worked-on leaf: the voxels o + (lx, ly, lz), 0 <= lx, ly, lz <= 8, the +1 faces from up to seven neighbours.
// put(l, off, i) for every voxel of the tile that a listed leaf holds: l = the leaf's index in the list, off = the voxel's offset
// in that leaf, i = (lx * 9 + ly) * 9 + lz = its place in the tile.  What no listed leaf holds is not visited.
template <typename Put>
inline void load_tile(const fluid_sdf_grid_t* g, const Org& o, Put put)
{
    for (int d = 0; d < 8; ++d) {
        const int dx = d >> 2, dy = (d >> 1) & 1, dz = d & 1;
        const long l = find_leaf(g, Org{o.x + 8 * dx, o.y + 8 * dy, o.z + 8 * dz});
        if (l < 0) continue;
        for (int x = 0; x < (dx ? 1 : 8); ++x)
            for (int y = 0; y < (dy ? 1 : 8); ++y)
                for (int z = 0; z < (dz ? 1 : 8); ++z) put(l, (x * 8 + y) * 8 + z, ((x + 8 * dx) * 9 + (y + 8 * dy)) * 9 + z + 8 * dz);
    }
}

}  // namespace
