// The box filter and offset of the level set on the host (include/fluid_hip.h, "liquid surface, smoothed") — no GPU, no HIP, no
// OpenVDB (the list's rules and the search in it: leaf_list.h).  fluid_sdf_filter applies the definition to a leaf list, every unlisted leaf and everything outside the grid
// being +bg: how a decomposed run smooths its merged surface (after fluid_sdf_grids_merge, before fluid_write_vdb_sdf /
// fluid_sdf_mesh), and the second implementation the kernels (kernels_sdf_filter.hip) are compared with.  Pass by pass, leaf by
// leaf: the leaf's 8 x 8 x (8 + 2W) values along the pass's axis, the two neighbour leaves found by bisection in the sorted list;
// the passes alternate between the caller's array and one scratch array of the same size, so that the last one writes the caller's.
// fluid_sdf_filter_tracked ("liquid surface, renormalised") is the same for the tracked filter: the box passes above, a
// normalisation pass that finds the six face neighbours by bisection (the per-voxel arithmetic is sdf_track_def.h's, shared with
// kernels_sdf_track.hip, or under FLUID_SDF_TRACK_HJWENO5 sdf_weno_def.h's, shared with kernels_sdf_weno.hip, the same six
// neighbours read three planes deep), the trim on masks of its own, and the list compacted to the leaves that still hold something.
// fluid_sdf_filter_grown ("liquid surface, grown band") is the tracked filter whose every track begins with a dilation of the
// masks (the word arithmetic is sdf_grow_def.h's, shared with kernels_sdf_grow.hip): the list is a working copy that the dilation
// lengthens by the unlisted face neighbours it activates voxels in, and the attributes travel with it.
// fluid_sdf_flow ("liquid surface, flows") is all three forms for a filter kind: the box passes, or one pass per iteration of a
// median, Laplacian or mean-curvature flow (the per-voxel arithmetic is sdf_flow_def.h's, shared with kernels_sdf_flow.hip) on the
// leaf's (8 + 2H)^3 tile, the 26 neighbour leaves found by bisection.
// All four run the one schedule of sdf_filter_plan.h (the order of passes, offset steps and tracks, and the arguments' limits,
// shared with fluid_sdf.hip); the tracked, the grown and the flow function are one entry path (band_filter: the refusals, then
// run_band on one working list, Band, then copy_out's one rule for which leaves stay listed) and differ in the arguments they fix:
// the kind, the dilation and what travels with the band.  A leaf's face neighbours in the list are found in one place
// (face_neighbours).
// Arithmetic: float, no contraction (x86-64 has none without -mfma; the builds state -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "leaf_list.h"
#include "sdf_filter_plan.h"
#include "sdf_flow_def.h"
#include "sdf_grow_def.h"
#include "sdf_weno_def.h"

namespace {

// the origin of the face neighbour of the leaf at o on axis a: side 0 = -1, 1 = +1
inline Org face_org(const Org& o, int a, int side)
{
    Org q = o;
    (a == 0 ? q.x : a == 1 ? q.y : q.z) += side ? LEAF : -LEAF;
    return q;
}

// the six face neighbours of the leaf at o as indices in g's list, -1 where unlisted: such a leaf reads as +bg
void face_neighbours(const fluid_sdf_grid_t* g, const Org& o, long nb[3][2])
{
    for (int a = 0; a < 3; ++a)
        for (int side = 0; side < 2; ++side) nb[a][side] = find_leaf(g, face_org(o, a, side));
}

// one pass of width W along `axis`: src -> dst (512 per leaf, the list's order); `off` is added to the active voxels' results
void box_pass(const fluid_sdf_grid_t* g, int axis, int W, float off, const float* src, float* dst)
{
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const float bg = g->background, frac = 1.0f / (float)(2 * W + 1);
    static const int stride[3] = {64, 8, 1};
    const int sa = stride[axis];
    float line[LEAF + 8];
    for (long l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        long nb[3][2];
        face_neighbours(g, org_of(g, l), nb);
        const long lm = nb[axis][0], lp = nb[axis][1];
        const float* v = src + 512 * (size_t)l;
        const float* vm = lm >= 0 ? src + 512 * (size_t)lm : nullptr;
        const float* vp = lp >= 0 ? src + 512 * (size_t)lp : nullptr;
        const uint64_t* mask = g->active + 8 * (size_t)l;
        float* out = dst + 512 * (size_t)l;
        // the 64 lines of the leaf along the axis: `base` = the offset of the line's first voxel
        for (int uv = 0; uv < 64; ++uv) {
            const int u = uv >> 3, w = uv & 7;
            const int base = axis == 0 ? u * 8 + w : axis == 1 ? u * 64 + w : u * 64 + w * 8;
            // the two other coordinates of the line: inside the grid?
            int c[3] = {o[0] + (base >> 6), o[1] + ((base >> 3) & 7), o[2] + (base & 7)};
            bool in_line = true;
            for (int a = 0; a < 3; ++a)
                if (a != axis) in_line = in_line && c[a] >= lo && c[a] <= hi;
            for (int k = -W; k < LEAF + W; ++k) {
                const int ca = o[axis] + k;
                float x = bg;
                if (in_line && ca >= lo && ca <= hi) {
                    if (k < 0) x = vm ? vm[base + (k + LEAF) * sa] : bg;
                    else if (k >= LEAF) x = vp ? vp[base + (k - LEAF) * sa] : bg;
                    else x = v[base + k * sa];
                }
                line[k + W] = x;
            }
            for (int k = 0; k < LEAF; ++k) {
                const int at = base + k * sa, ca = o[axis] + k;
                float r = v[at];
                if (in_line && ca >= lo && ca <= hi && ((mask[at >> 6] >> (at & 63)) & 1ull)) {
                    float s = 0.0f;
                    for (int i = 0; i <= 2 * W; ++i) s = s + line[k + i];
                    r = s * frac;
                    if (off != 0.0f) r = r + off;
                }
                out[at] = r;
            }
        }
    }
}

inline bool in_grid(const fluid_sdf_grid_t* g, const int32_t* o, int at)
{
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const int c[3] = {o[0] + (at >> 6), o[1] + ((at >> 3) & 7), o[2] + (at & 7)};
    return c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
}
inline bool is_active(const uint64_t* mask, size_t l, int at) { return (mask[8 * l + (at >> 6)] >> (at & 63)) & 1ull; }

// the offset, or a step of it: added to the active voxels inside the grid (g->origin and g->active; val: 512 per leaf)
void add_active(const fluid_sdf_grid_t* g, float step, float* val)
{
    for (size_t l = 0; l < (size_t)g->n_leaves; ++l)
        for (int at = 0; at < 512; ++at)
            if (is_active(g->active, l, at) && in_grid(g, g->origin + 3 * l, at)) val[512 * l + at] = val[512 * l + at] + step;
}

// ---- "liquid surface, flows": the arithmetic is sdf_flow_def.h's; here the 26 neighbour leaves and the (8 + 2H)^3 tile -------------
// one pass of a median (width W), Laplacian or mean-curvature flow: src -> dst (512 per leaf, the list's order); `off` is added to
// the active voxels' results
void flow_pass(const fluid_sdf_grid_t* g, int kind, int W, float dx, float off, const float* src, float* dst)
{
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const float bg = g->background;
    const fdef::Consts k = fdef::consts(dx);
    const int H = kind == FLUID_SDF_FILTER_MEDIAN ? W : 1, S = LEAF + 2 * H;
    std::vector<float> tile((size_t)S * S * S);
    for (long l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        const float* nb[27];   // the leaves around this one ((dx + 1) * 9 + (dy + 1) * 3 + dz + 1), nullptr where unlisted
        for (int d = 0; d < 27; ++d) {
            const long q = d == 13 ? l : find_leaf(g, Org{o[0] + (d / 9 - 1) * LEAF, o[1] + (d / 3 % 3 - 1) * LEAF, o[2] + (d % 3 - 1) * LEAF});
            nb[d] = q >= 0 ? src + 512 * (size_t)q : nullptr;
        }
        // the tile: voxel o + (X - H, Y - H, Z - H) at (X * S + Y) * S + Z; +bg outside the grid and in unlisted leaves
        for (int X = 0; X < S; ++X)
            for (int Y = 0; Y < S; ++Y)
                for (int Z = 0; Z < S; ++Z) {
                    const int r[3] = {X - H, Y - H, Z - H};
                    int d = 0, at = 0;
                    bool in = true;
                    for (int a = 0; a < 3; ++a) {
                        const int side = r[a] < 0 ? -1 : r[a] >= LEAF ? 1 : 0, c = o[a] + r[a];
                        in = in && c >= lo && c <= hi;
                        d = d * 3 + side + 1;
                        at = at * 8 + (r[a] - side * LEAF);
                    }
                    tile[((size_t)X * S + Y) * S + Z] = in && nb[d] ? nb[d][at] : bg;
                }
        const float* v = src + 512 * (size_t)l;
        float* out = dst + 512 * (size_t)l;
        for (int at = 0; at < 512; ++at) {
            out[at] = v[at];
            if (!is_active(g->active, (size_t)l, at) || !in_grid(g, o, at)) continue;
            const int x = at >> 6, y = (at >> 3) & 7, z = at & 7;
            auto T = [&](int i, int j, int m) { return tile[((size_t)(x + H + i) * S + (y + H + j)) * S + (z + H + m)]; };
            float r;
            if (kind == FLUID_SDF_FILTER_MEDIAN) {
                uint32_t keys[fdef::median_count(2)];
                int m = 0;
                for (int i = -W; i <= W; ++i)
                    for (int j = -W; j <= W; ++j)
                        for (int q = -W; q <= W; ++q) {
                            const float f = T(i, j, q);
                            uint32_t bits;
                            memcpy(&bits, &f, 4);
                            keys[m++] = fdef::median_key(bits);
                        }
                const uint32_t bits = fdef::median_bits(fdef::median_select(m, (m - 1) >> 1, [&](int i) { return keys[i]; }));
                memcpy(&r, &bits, 4);
            } else if (kind == FLUID_SDF_FILTER_LAPLACIAN) {
                r = fdef::laplacian_value(v[at], T(-1, 0, 0), T(1, 0, 0), T(0, -1, 0), T(0, 1, 0), T(0, 0, -1), T(0, 0, 1), k.invdx2, k.dt_lap);
            } else {
                const fdef::Edges e{T(1, 1, 0), T(1, -1, 0), T(-1, -1, 0), T(-1, 1, 0), T(1, 0, 1), T(1, 0, -1), T(-1, 0, -1), T(-1, 0, 1),
                                    T(0, 1, 1), T(0, 1, -1), T(0, -1, -1), T(0, -1, 1)};
                r = fdef::curvature_value(v[at], T(-1, 0, 0), T(1, 0, 0), T(0, -1, 0), T(0, 1, 0), T(0, 0, -1), T(0, 0, 1), e, k.invdx2, k.dt_curv);
            }
            if (off != 0.0f) r = r + off;
            out[at] = r;
        }
    }
}

// ---- "liquid surface, renormalised": the arithmetic is sdf_track_def.h's, or three planes deep ("HJWENO5") sdf_weno_def.h's; here
// the neighbours, the masks and the list ------------------------------------------------------------------------------------------
// one normalisation pass src -> dst (512 per leaf, the list's order) that reads D values either way on every axis: D = 1
// tdef::track_value, D = 3 wdef::track_value_weno; g->active is the mask as it is now
template <int D> void norm_pass(const fluid_sdf_grid_t* g, float dx, const float* src, float* dst)
{
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const float bg = g->background, dt = dx * 0.3f, inv = 1.0f / dx;
    static const int stride[3] = {64, 8, 1};
    for (long l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        long nb[3][2];
        face_neighbours(g, org_of(g, l), nb);
        const float* v = src + 512 * (size_t)l;
        float* out = dst + 512 * (size_t)l;
        for (int at = 0; at < 512; ++at) {
            out[at] = v[at];
            if (!is_active(g->active, (size_t)l, at) || !in_grid(g, o, at)) continue;
            const int c[3] = {at >> 6, (at >> 3) & 7, at & 7};
            float u[3][2 * D + 1];
            for (int a = 0; a < 3; ++a)
                for (int d = -D; d <= D; ++d) {
                    const int k = c[a] + d, ca = o[a] + k;
                    float x = bg;
                    if (ca >= lo && ca <= hi) {
                        if (k < 0) x = nb[a][0] >= 0 ? src[512 * (size_t)nb[a][0] + at + (d + LEAF) * stride[a]] : bg;
                        else if (k >= LEAF) x = nb[a][1] >= 0 ? src[512 * (size_t)nb[a][1] + at + (d - LEAF) * stride[a]] : bg;
                        else x = v[at + d * stride[a]];
                    }
                    u[a][d + D] = x;
                }
            if constexpr (D == 1) out[at] = tdef::track_value(v[at], u[0][0], u[0][2], u[1][0], u[1][2], u[2][0], u[2][2], dt, inv);
            else out[at] = wdef::track_value_weno(u[0], u[1], u[2], dt, inv);
        }
    }
}

void trim_pass(const fluid_sdf_grid_t* g, float* val, uint64_t* mask)
{
    for (long l = 0; l < g->n_leaves; ++l)
        for (int at = 0; at < 512; ++at) {
            uint64_t& w = mask[8 * (size_t)l + (at >> 6)];
            if (!((w >> (at & 63)) & 1ull) || !in_grid(g, g->origin + 3 * (size_t)l, at)) continue;
            float& x = val[512 * (size_t)l + at];
            const int cls = tdef::trim_class(x, g->background);
            if (cls == 0) continue;
            x = cls < 0 ? -g->background : g->background;
            w &= ~(1ull << (at & 63));
        }
}

// a band to track in: a background and a half width to take dx from
bool band_ok(const fluid_sdf_grid_t* g) { return g->background > 0.0f && g->half_width > 0.0f; }

// the list carries bg = dx * half_width, not dx: the quotient, or its float neighbour whose product gives bg back
float list_dx(const fluid_sdf_grid_t* g)
{
    const float bg = g->background, dx = bg / g->half_width;
    for (const float c : {dx, std::nextafter(dx, 0.0f), std::nextafter(dx, INFINITY)})
        if (c * g->half_width == bg) return c;
    return dx;
}

// does an input array (nl leaves) overlap an output array (cap leaves)?  {pointer, bytes per leaf}; a null pointer overlaps nothing
struct Arr { const void* p; size_t per_leaf; };
bool overlap(std::initializer_list<Arr> in, size_t nl, std::initializer_list<Arr> out, size_t cap)
{
    for (const Arr& a : in)
        for (const Arr& b : out) {
            const uintptr_t a0 = (uintptr_t)a.p, a1 = a0 + a.per_leaf * nl, b0 = (uintptr_t)b.p, b1 = b0 + b.per_leaf * cap;
            if (a.p && b.p && nl && cap && a0 < b1 && b0 < a1) return true;
        }
    return false;
}

// ---- the working list of the tracked and the grown filter, which a dilation can lengthen ------------------------------------------
struct Band {
    std::vector<int32_t> org;      // 3 per leaf, ascending
    std::vector<int32_t> from;     // per leaf: its index in the caller's list (`kept`), -1 for a leaf a dilation added
    std::vector<uint64_t> mask;    // 8 per leaf
    std::vector<float> val[2];     // 512 per leaf: the passes' ping-pong, `at` = the one that holds the values
    int at = 0;
    bool attr = false;             // "liquid surface, grown band": the attributes travel with the band
    std::vector<uint32_t> id;      // 512 per leaf
    std::vector<float> vel;        // 3 x 512 per leaf
    size_t leaves() const { return org.size() / 3; }
    Band() = default;
    Band(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* a) : org(g->origin, g->origin + 3 * (size_t)g->n_leaves), from((size_t)g->n_leaves),
        mask(g->active, g->active + 8 * (size_t)g->n_leaves), attr(a != nullptr)
    {
        const size_t nl = leaves();
        for (size_t l = 0; l < nl; ++l) from[l] = (int32_t)l;
        val[0].assign(g->values, g->values + 512 * nl), val[1].resize(512 * nl);
        if (a) id.assign(a->id, a->id + 512 * nl), vel.assign(a->velocity, a->velocity + 1536 * nl);
    }
};

// One dilation of the band's masks (the mask words: sdf_grow_def.h).  `cur` describes the band as it is (origin, active, n_leaves
// point into b) and is pointed at the new arrays on return.  Leaf by leaf: the listed leaves, then the unlisted face neighbours of
// listed leaves, which join the list (+bg, NO_ID, +0) when a voxel of theirs becomes active.
void dilate(fluid_sdf_grid_t* cur, Band& b)
{
    const int lo = -(cur->n / 2), hi = lo + cur->n - 1, L0 = floor_to(lo, LEAF), L1 = floor_to(hi, LEAF);
    const size_t nl = b.leaves();
    std::vector<uint64_t> eff(8 * nl);   // the masks as the definition reads them: nothing outside the grid is active
    for (size_t l = 0; l < nl; ++l)
        for (int x = 0; x < 8; ++x)
            eff[8 * l + x] = b.mask[8 * l + x] & gdef::grid_word(b.org[3 * l] + x, b.org[3 * l + 1], b.org[3 * l + 2], lo, hi);
    // the new bits of the leaf at o (self = its index, -1: unlisted), and for each its id and velocity (into id512 / vel1536)
    auto grow_leaf = [&](const Org& o, long self, uint64_t fresh[8], uint32_t* id512, float* vel1536) {
        long nb3[3][2];
        face_neighbours(cur, o, nb3);
        const long* nb = &nb3[0][0];   // direction d = 2 * axis + side: -x +x -y +y -z +z
        auto word = [&](long l, int x) { return l >= 0 ? eff[8 * (size_t)l + x] : 0ull; };
        bool any = false;
        for (int x = 0; x < 8; ++x) {
            uint64_t c[6];
            gdef::neighbours(word(self, x), x > 0 ? word(self, x - 1) : word(nb[0], 7), x < 7 ? word(self, x + 1) : word(nb[1], 0), word(nb[2], x),
                             word(nb[3], x), word(nb[4], x), word(nb[5], x), c);
            fresh[x] = (c[0] | c[1] | c[2] | c[3] | c[4] | c[5]) & gdef::grid_word(o.x + x, o.y, o.z, lo, hi) & ~word(self, x);
            any = any || fresh[x];
            if (!b.attr) continue;
            for (int bit = 0; bit < 64; ++bit) {
                if (!((fresh[x] >> bit) & 1ull)) continue;
                int d = 0;
                while (!((c[d] >> bit) & 1ull)) ++d;   // the first neighbour in the order -x +x -y +y -z +z that was active
                const int at = x * 64 + bit, from = gdef::neighbour_offset(at, d);
                const size_t src = (size_t)(gdef::neighbour_crosses(at, d) ? nb[d] : self);
                id512[at] = b.id[512 * src + from];
                for (int a = 0; a < 3; ++a) vel1536[512 * a + at] = b.vel[1536 * src + 512 * a + from];
            }
        }
        return any;
    };
    // the unlisted face neighbours of the listed leaves, inside the grid's leaves
    std::vector<Org> cand;
    for (size_t l = 0; l < nl; ++l) {
        const Org o = org_of(cur, (long)l);
        long nb[3][2];
        face_neighbours(cur, o, nb);
        for (int a = 0; a < 3; ++a)
            for (int side = 0; side < 2; ++side) {
                const Org q = face_org(o, a, side);
                const int32_t k = a == 0 ? q.x : a == 1 ? q.y : q.z;
                if (k >= L0 && k <= L1 && nb[a][side] < 0) cand.push_back(q);
            }
    }
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    std::vector<Org> add;
    std::vector<uint64_t> add_mask;
    std::vector<uint32_t> add_id;
    std::vector<float> add_vel;
    for (const Org& o : cand) {
        uint64_t fresh[8];
        uint32_t id512[512];
        float vel1536[1536];
        for (int i = 0; i < 512; ++i) id512[i] = FLUID_SDF_NO_ID;
        for (int i = 0; i < 1536; ++i) vel1536[i] = 0.0f;
        if (!grow_leaf(o, -1, fresh, id512, vel1536)) continue;
        add.push_back(o);
        add_mask.insert(add_mask.end(), fresh, fresh + 8);
        if (b.attr) add_id.insert(add_id.end(), id512, id512 + 512), add_vel.insert(add_vel.end(), vel1536, vel1536 + 1536);
    }
    // the listed leaves: a new voxel's source was active before, so it is never one this loop writes
    std::vector<uint64_t> grown(8 * nl);
    for (size_t l = 0; l < nl; ++l)
        grow_leaf(Org{b.org[3 * l], b.org[3 * l + 1], b.org[3 * l + 2]}, (long)l, &grown[8 * l], b.attr ? &b.id[512 * l] : nullptr,
                  b.attr ? &b.vel[1536 * l] : nullptr);
    for (size_t i = 0; i < 8 * nl; ++i) b.mask[i] |= grown[i];
    if (!add.empty()) {   // merge the two ascending lists
        Band m;
        m.at = b.at, m.attr = b.attr;
        const size_t total = nl + add.size();
        m.org.reserve(3 * total), m.from.reserve(total), m.mask.reserve(8 * total), m.val[0].reserve(512 * total), m.val[1].resize(512 * total);
        if (b.attr) m.id.reserve(512 * total), m.vel.reserve(1536 * total);
        const std::vector<float>& v = b.val[b.at];
        for (size_t i = 0, k = 0; i < nl || k < add.size();) {
            const bool old = k == add.size() || (i < nl && Org{b.org[3 * i], b.org[3 * i + 1], b.org[3 * i + 2]} < add[k]);
            if (old) {
                m.org.insert(m.org.end(), &b.org[3 * i], &b.org[3 * i] + 3);
                m.from.push_back(b.from[i]);
                m.mask.insert(m.mask.end(), &b.mask[8 * i], &b.mask[8 * i] + 8);
                m.val[0].insert(m.val[0].end(), &v[512 * i], &v[512 * i] + 512);
                if (b.attr) m.id.insert(m.id.end(), &b.id[512 * i], &b.id[512 * i] + 512), m.vel.insert(m.vel.end(), &b.vel[1536 * i], &b.vel[1536 * i] + 1536);
                ++i;
            } else {
                const int32_t o[3] = {add[k].x, add[k].y, add[k].z};
                m.org.insert(m.org.end(), o, o + 3);
                m.from.push_back(-1);
                m.mask.insert(m.mask.end(), &add_mask[8 * k], &add_mask[8 * k] + 8);
                m.val[0].insert(m.val[0].end(), 512, cur->background);
                if (b.attr) m.id.insert(m.id.end(), &add_id[512 * k], &add_id[512 * k] + 512), m.vel.insert(m.vel.end(), &add_vel[1536 * k], &add_vel[1536 * k] + 1536);
                ++k;
            }
        }
        m.at = 0;
        b = std::move(m);
    }
    cur->n_leaves = (int32_t)b.leaves();
    cur->origin = b.org.data();
    cur->active = b.mask.data();
    cur->values = nullptr;
}

// trim_pass, which also takes the id and velocity from the voxels it deactivates
void trim_pass_attr(const fluid_sdf_grid_t* g, Band& b)
{
    if (!b.attr) return trim_pass(g, b.val[b.at].data(), b.mask.data());
    const std::vector<uint64_t> before = b.mask;
    trim_pass(g, b.val[b.at].data(), b.mask.data());
    for (size_t l = 0; l < b.leaves(); ++l)
        for (int at = 0; at < 512; ++at)
            if (((before[8 * l + (at >> 6)] ^ b.mask[8 * l + (at >> 6)]) >> (at & 63)) & 1ull) {
                b.id[512 * l + at] = FLUID_SDF_NO_ID;
                for (int a = 0; a < 3; ++a) b.vel[1536 * l + 512 * a + at] = 0.0f;
            }
}

// The filter of `kind` on a band (the schedule: sdf_filter_plan.h), tracked or not: a track is the dilation when growing, N
// normalisation passes and the trim.  True when a trim ran, which is when leaves can have left the list.
bool run_band(const fluid_sdf_grid_t* g, Band& b, int kind, const fluid_sdf_filter_t* f, bool tracked, int N, bool trim, bool grow, int scheme)
{
    fluid_sdf_grid_t cur = *g;   // the band as it is now: dilate() keeps it pointing into b
    cur.origin = b.org.data(), cur.active = b.mask.data(), cur.values = nullptr;
    const float dx = tracked || plan::kind_needs_dx(kind) ? list_dx(g) : 0.0f;
    bool trimmed = false;
    plan::run(
        kind, *f, dx, tracked,
        [&](int axis, int W, float off) {
            box_pass(&cur, axis, W, off, b.val[b.at].data(), b.val[1 - b.at].data());
            b.at = 1 - b.at;
        },
        [&](int kd, int W, float off) {
            flow_pass(&cur, kd, W, dx, off, b.val[b.at].data(), b.val[1 - b.at].data());
            b.at = 1 - b.at;
        },
        [&](float step) { add_active(&cur, step, b.val[b.at].data()); },
        [&]() {
            if (grow) dilate(&cur, b);
            for (int i = 0; i < N; ++i) {
                if (scheme == FLUID_SDF_TRACK_HJWENO5) norm_pass<3>(&cur, dx, b.val[b.at].data(), b.val[1 - b.at].data());
                else norm_pass<1>(&cur, dx, b.val[b.at].data(), b.val[1 - b.at].data());
                b.at = 1 - b.at;
            }
            if (trim) trim_pass_attr(&cur, b), trimmed = true;
        });
    return trimmed;
}

// The band into the caller's arrays (origin == nullptr: the count alone).  Listed: every leaf when no trim ran, else a leaf with an
// in-grid voxel that is anything but inactive +bg.  The count, or -FLUID_ERR_ARG with nothing written when cap_leaves is too small.
int64_t copy_out(const fluid_sdf_grid_t* g, const Band& b, bool trimmed, int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active,
                 int32_t* kept, uint32_t* id, float* velocity)
{
    const float* v = b.val[b.at].data();
    std::vector<size_t> keep;
    for (size_t l = 0; l < b.leaves(); ++l) {
        bool any = !trimmed;
        for (int at = 0; at < 512 && !any; ++at) any = in_grid(g, &b.org[3 * l], at) && (is_active(b.mask.data(), l, at) || v[512 * l + at] != g->background);
        if (any) keep.push_back(l);
    }
    if (!origin) return (int64_t)keep.size();
    if (cap_leaves < (int64_t)keep.size()) return -FLUID_ERR_ARG;
    for (size_t i = 0; i < keep.size(); ++i) {
        const size_t l = keep[i];
        memcpy(origin + 3 * i, &b.org[3 * l], 3 * sizeof(int32_t));
        memcpy(values + 512 * i, v + 512 * l, 512 * sizeof(float));
        memcpy(active + 8 * i, &b.mask[8 * l], 8 * sizeof(uint64_t));
        if (kept) kept[i] = b.from[l];
        if (b.attr) memcpy(id + 512 * i, &b.id[512 * l], 512 * sizeof(uint32_t)), memcpy(velocity + 1536 * i, &b.vel[1536 * l], 1536 * sizeof(float));
    }
    return (int64_t)keep.size();
}

// The tracked, the grown and the flow entry point: everything that can be refused first; the result is made in a band of our own
// and copied last.  The count of listed leaves, or -FLUID_ERR_ARG with nothing written.
int64_t band_filter(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* attr, int32_t kind, const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t,
                    int32_t grow, int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active, int32_t* kept, uint32_t* id, float* velocity)
{
    if (check_list(g) != FLUID_OK || !plan::filter_ok(f) || !plan::kind_ok(kind) || !plan::width_ok(kind, f->width)) return -FLUID_ERR_ARG;
    if (!plan::track_ok(t) || (grow != 0 && grow != 1) || (grow && !plan::grow_ok(t))) return -FLUID_ERR_ARG;
    const bool tracked = grow || plan::tracking(t);
    if ((tracked || plan::kind_needs_dx(kind)) && !band_ok(g)) return -FLUID_ERR_ARG;
    if (grow ? !plan::grown_offset_ok((float)f->offset, list_dx(g)) : tracked && !plan::tracked_offset_ok((float)f->offset, g->background))
        return -FLUID_ERR_ARG;
    const size_t nl = (size_t)g->n_leaves;
    if (attr && (attr->n_leaves != g->n_leaves || (nl > 0 && (!attr->id || !attr->velocity)))) return -FLUID_ERR_ARG;
    const bool count_only = !origin && !values && !active && !id && !velocity;
    if (!count_only) {
        if (!origin || !values || !active || cap_leaves < 0) return -FLUID_ERR_ARG;
        if (attr ? (!id || !velocity) : (id || velocity)) return -FLUID_ERR_ARG;
        if (overlap({{g->origin, 12}, {g->values, 2048}, {g->active, 64}, {attr ? attr->id : nullptr, 2048}, {attr ? attr->velocity : nullptr, 6144}}, nl,
                    {{origin, 12}, {values, 2048}, {active, 64}, {kept, 4}, {id, 2048}, {velocity, 6144}}, (size_t)cap_leaves))
            return -FLUID_ERR_ARG;
    }
    if (nl == 0) return 0;
    if (!tracked && count_only) return g->n_leaves;
    Band b(g, attr);
    const bool trimmed = run_band(g, b, kind, f, tracked, tracked ? t->normalize : 0, tracked && t->trim != 0, grow != 0, tracked ? t->scheme : FLUID_SDF_TRACK_FIRST_BIAS);
    return copy_out(g, b, trimmed, cap_leaves, origin, values, active, kept, id, velocity);
}

}  // namespace

extern "C" {

int fluid_sdf_filter(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, float* values)
{
    if (check_list(g) != FLUID_OK || !plan::filter_ok(f)) return FLUID_ERR_ARG;
    const size_t count = 512 * (size_t)g->n_leaves;
    if (count == 0) return FLUID_OK;
    if (!values || overlap({{g->values, 2048}}, (size_t)g->n_leaves, {{values, 2048}}, (size_t)g->n_leaves)) return FLUID_ERR_ARG;
    const int passes = plan::passes(FLUID_SDF_FILTER_BOX, *f);
    if (passes == 0) memcpy(values, g->values, count * sizeof(float));
    std::vector<float> scratch(passes ? count : 0);
    const float* src = g->values;
    int k = 0;
    plan::run(
        FLUID_SDF_FILTER_BOX, *f, 0.0f, false,
        [&](int axis, int W, float off) {
            float* dst = ((passes - 1 - k++) & 1) ? scratch.data() : values;   // the last pass writes `values`
            box_pass(g, axis, W, off, src, dst);
            src = dst;
        },
        [](int, int, float) {}, [&](float off) { add_active(g, off, values); }, [] {});
    return FLUID_OK;
}

int64_t fluid_sdf_filter_tracked(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t, int64_t cap_leaves,
                                 int32_t* origin, float* values, uint64_t* active, int32_t* kept)
{
    return band_filter(g, nullptr, FLUID_SDF_FILTER_BOX, f, t, 0, cap_leaves, origin, values, active, kept, nullptr, nullptr);
}

int64_t fluid_sdf_filter_grown(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* attr, const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t,
                               int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active, uint32_t* id, float* velocity)
{
    return band_filter(g, attr, FLUID_SDF_FILTER_BOX, f, t, 1, cap_leaves, origin, values, active, nullptr, id, velocity);
}

int64_t fluid_sdf_flow(const fluid_sdf_grid_t* g, const fluid_sdf_attr_t* attr, int32_t kind, const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t,
                       int32_t grow, int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active, uint32_t* id, float* velocity)
{
    return band_filter(g, attr, kind, f, t, grow, cap_leaves, origin, values, active, nullptr, id, velocity);
}

}  // extern "C"
