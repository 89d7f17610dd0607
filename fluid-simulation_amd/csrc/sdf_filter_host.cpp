// The box filter and offset of the level set on the host (include/fluid_hip.h, "liquid surface, smoothed") — no GPU, no HIP, no
// OpenVDB (the list's rules and the search in it: leaf_list.h).  fluid_sdf_filter applies the definition to a leaf list, every unlisted leaf and everything outside the grid
// being +bg: how a decomposed run smooths its merged surface (after fluid_sdf_grids_merge, before fluid_write_vdb_sdf /
// fluid_sdf_mesh), and the second implementation the kernels (kernels_sdf_filter.hip) are compared with.  Pass by pass, leaf by
// leaf: the leaf's 8 x 8 x (8 + 2W) values along the pass's axis, the two neighbour leaves found by bisection in the sorted list;
// the passes alternate between the caller's array and one scratch array of the same size, so that the last one writes the caller's.
// fluid_sdf_filter_tracked ("liquid surface, renormalised") is the same for the tracked filter: the box passes above, a
// normalisation pass that finds the six face neighbours by bisection (the per-voxel arithmetic is sdf_track_def.h's, shared with
// kernels_sdf_track.hip), the trim on masks of its own, and the list compacted to the leaves that still hold something.
// Arithmetic: float, no contraction (x86-64 has none without -mfma; the builds state -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "leaf_list.h"
#include "sdf_track_def.h"

namespace {

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
        Org om{o[0], o[1], o[2]}, op = om;
        (axis == 0 ? om.x : axis == 1 ? om.y : om.z) -= LEAF;
        (axis == 0 ? op.x : axis == 1 ? op.y : op.z) += LEAF;
        const long lm = find_leaf(g, om), lp = find_leaf(g, op);
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

bool filter_ok(const fluid_sdf_filter_t* f)
{
    return f && f->width >= 1 && f->width <= 4 && f->iterations >= 0 && f->iterations <= 16 && std::isfinite(f->offset) && std::isfinite((float)f->offset);
}

// ---- "liquid surface, renormalised": the arithmetic is sdf_track_def.h's; here the neighbours, the masks and the list ----------
inline bool in_grid(const fluid_sdf_grid_t* g, const int32_t* o, int at)
{
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const int c[3] = {o[0] + (at >> 6), o[1] + ((at >> 3) & 7), o[2] + (at & 7)};
    return c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
}

// one normalisation pass src -> dst (512 per leaf, the list's order); g->active is the mask as it is now
void norm_pass(const fluid_sdf_grid_t* g, float dx, const float* src, float* dst)
{
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const float bg = g->background, dt = dx * 0.3f, inv = 1.0f / dx;
    static const int stride[3] = {64, 8, 1};
    for (long l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        const float* nb[3][2];   // the face neighbours' values, nullptr where unlisted
        for (int a = 0; a < 3; ++a)
            for (int side = 0; side < 2; ++side) {
                Org q{o[0], o[1], o[2]};
                (a == 0 ? q.x : a == 1 ? q.y : q.z) += side ? LEAF : -LEAF;
                const long k = find_leaf(g, q);
                nb[a][side] = k >= 0 ? src + 512 * (size_t)k : nullptr;
            }
        const float* v = src + 512 * (size_t)l;
        const uint64_t* mask = g->active + 8 * (size_t)l;
        float* out = dst + 512 * (size_t)l;
        for (int at = 0; at < 512; ++at) {
            out[at] = v[at];
            if (!((mask[at >> 6] >> (at & 63)) & 1ull) || !in_grid(g, o, at)) continue;
            const int c[3] = {at >> 6, (at >> 3) & 7, at & 7};
            float n6[3][2];
            for (int a = 0; a < 3; ++a)
                for (int side = 0; side < 2; ++side) {
                    const int k = c[a] + (side ? 1 : -1), ca = o[a] + k;
                    float x = bg;
                    if (ca >= lo && ca <= hi) {
                        if (k < 0) x = nb[a][0] ? nb[a][0][at + 7 * stride[a]] : bg;
                        else if (k >= LEAF) x = nb[a][1] ? nb[a][1][at - 7 * stride[a]] : bg;
                        else x = v[at + (side ? stride[a] : -stride[a])];
                    }
                    n6[a][side] = x;
                }
            out[at] = tdef::track_value(v[at], n6[0][0], n6[0][1], n6[1][0], n6[1][1], n6[2][0], n6[2][1], dt, inv);
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

bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a && b && na && nb && a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int fluid_sdf_filter(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, float* values)
{
    if (check_list(g) != FLUID_OK || !filter_ok(f)) return FLUID_ERR_ARG;
    const size_t count = 512 * (size_t)g->n_leaves;
    if (count == 0) return FLUID_OK;
    if (!values) return FLUID_ERR_ARG;
    const uintptr_t a0 = (uintptr_t)g->values, a1 = a0 + count * sizeof(float), b0 = (uintptr_t)values, b1 = b0 + count * sizeof(float);
    if (a0 < b1 && b0 < a1) return FLUID_ERR_ARG;
    const int lo = -(g->n / 2), hi = lo + g->n - 1;
    const float off = (float)f->offset;
    const int passes = 3 * f->iterations;
    if (passes == 0) {
        memcpy(values, g->values, count * sizeof(float));
        if (off != 0.0f)
            for (long l = 0; l < g->n_leaves; ++l) {
                const int32_t* o = g->origin + 3 * (size_t)l;
                for (int at = 0; at < 512; ++at) {
                    const int c[3] = {o[0] + (at >> 6), o[1] + ((at >> 3) & 7), o[2] + (at & 7)};
                    const bool in = c[0] >= lo && c[0] <= hi && c[1] >= lo && c[1] <= hi && c[2] >= lo && c[2] <= hi;
                    if (in && ((g->active[8 * (size_t)l + (at >> 6)] >> (at & 63)) & 1ull)) values[512 * (size_t)l + at] = values[512 * (size_t)l + at] + off;
                }
            }
        return FLUID_OK;
    }
    std::vector<float> scratch(count);
    static const int axes[3] = {0, 2, 1};   // the library's order: x, z, y
    const float* src = g->values;
    for (int k = 0; k < passes; ++k) {
        float* dst = ((passes - 1 - k) & 1) ? scratch.data() : values;   // the last pass writes `values`
        box_pass(g, axes[k % 3], f->width, k == passes - 1 ? off : 0.0f, src, dst);
        src = dst;
    }
    return FLUID_OK;
}

int64_t fluid_sdf_filter_tracked(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t, int64_t cap_leaves,
                                 int32_t* origin, float* values, uint64_t* active, int32_t* kept)
{
    // first pass: everything that can be refused, and the result in arrays of our own; second pass: the copy
    if (check_list(g) != FLUID_OK || !filter_ok(f)) return -FLUID_ERR_ARG;
    if (t && (t->normalize < 0 || t->normalize > tdef::MAX_PASSES || (t->trim != 0 && t->trim != 1) || t->scheme != FLUID_SDF_TRACK_FIRST_BIAS))
        return -FLUID_ERR_ARG;
    const int N = t ? t->normalize : 0;
    const bool trim = t && t->trim != 0, tracked = N > 0 || trim;
    const float off = (float)f->offset, bg = g->background;
    if (tracked && (std::fabs(off) > bg || !(bg > 0.0f) || !(g->half_width > 0.0f))) return -FLUID_ERR_ARG;
    const bool count_only = !origin && !values && !active;
    if (!count_only && (!origin || !values || !active || cap_leaves < 0)) return -FLUID_ERR_ARG;
    const size_t nl = (size_t)g->n_leaves, count = 512 * nl;
    if (!count_only) {
        const size_t cap = (size_t)cap_leaves;
        const void* in[3] = {g->origin, g->values, g->active};
        const size_t nin[3] = {12 * nl, 2048 * nl, 64 * nl};
        const void* out[4] = {origin, values, active, kept};
        const size_t nout[4] = {12 * cap, 2048 * cap, 64 * cap, 4 * cap};
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 4; ++k)
                if (overlaps(in[i], nin[i], out[k], nout[k])) return -FLUID_ERR_ARG;
    }
    if (nl == 0) return 0;
    std::vector<float> val(count);
    std::vector<uint64_t> mask(g->active, g->active + 8 * nl);
    std::vector<int32_t> keep(nl);
    for (size_t l = 0; l < nl; ++l) keep[l] = (int32_t)l;
    if (!tracked) {
        if (!count_only && cap_leaves < g->n_leaves) return -FLUID_ERR_ARG;
        if (count_only) return g->n_leaves;
        if (fluid_sdf_filter(g, f, val.data()) != FLUID_OK) return -FLUID_ERR_ARG;
    } else {
        std::vector<float> other(count);
        fluid_sdf_grid_t cur = *g;   // the list with the mask as it is now
        cur.active = mask.data();
        // the list carries bg = dx * half_width, not dx: the quotient, or its float neighbour whose product gives bg back
        float dx = bg / g->half_width;
        for (const float c : {dx, std::nextafter(dx, 0.0f), std::nextafter(dx, INFINITY)})
            if (c * g->half_width == bg) {
                dx = c;
                break;
            }
        memcpy(val.data(), g->values, count * sizeof(float));
        float *src = val.data(), *dst = other.data();
        bool trimmed = false;
        auto track = [&]() {
            for (int i = 0; i < N; ++i) {
                norm_pass(&cur, dx, src, dst);
                std::swap(src, dst);
            }
            if (trim) trim_pass(&cur, src, mask.data()), trimmed = true;
        };
        static const int axes[3] = {0, 2, 1};
        for (int k = 0; k < 3 * f->iterations; ++k) {
            box_pass(&cur, axes[k % 3], f->width, 0.0f, src, dst);
            std::swap(src, dst);
            if (k % 3 == 2) track();
        }
        const float a = std::fabs(off);
        float d = 0.0f;
        for (float delta; (delta = tdef::offset_step(a, d, dx)) != 0.0f;) {
            d = d + delta;
            const float step = std::copysign(delta, off);
            for (size_t l = 0; l < nl; ++l)
                for (int at = 0; at < 512; ++at)
                    if (((mask[8 * l + (at >> 6)] >> (at & 63)) & 1ull) && in_grid(g, g->origin + 3 * l, at)) src[512 * l + at] = src[512 * l + at] + step;
            track();
        }
        if (src != val.data()) memcpy(val.data(), src, count * sizeof(float));
        if (trimmed) {   // listed: an in-grid voxel that is anything but inactive +bg
            keep.clear();
            for (size_t l = 0; l < nl; ++l) {
                bool any = false;
                for (int at = 0; at < 512 && !any; ++at)
                    any = in_grid(g, g->origin + 3 * l, at) && (((mask[8 * l + (at >> 6)] >> (at & 63)) & 1ull) || val[512 * l + at] != bg);
                if (any) keep.push_back((int32_t)l);
            }
        }
        if (count_only) return (int64_t)keep.size();
        if (cap_leaves < (int64_t)keep.size()) return -FLUID_ERR_ARG;
    }
    for (size_t i = 0; i < keep.size(); ++i) {
        const size_t l = (size_t)keep[i];
        memcpy(origin + 3 * i, g->origin + 3 * l, 3 * sizeof(int32_t));
        memcpy(values + 512 * i, val.data() + 512 * l, 512 * sizeof(float));
        memcpy(active + 8 * i, mask.data() + 8 * l, 8 * sizeof(uint64_t));
        if (kept) kept[i] = keep[i];
    }
    return (int64_t)keep.size();
}

}  // extern "C"
