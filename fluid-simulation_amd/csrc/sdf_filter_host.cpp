// The box filter and offset of the level set on the host (include/fluid_hip.h, "liquid surface, smoothed") — no GPU, no HIP, no
// OpenVDB (the list's rules and the search in it: leaf_list.h).  fluid_sdf_filter applies the definition to a leaf list, every unlisted leaf and everything outside the grid
// being +bg: how a decomposed run smooths its merged surface (after fluid_sdf_grids_merge, before fluid_write_vdb_sdf /
// fluid_sdf_mesh), and the second implementation the kernels (kernels_sdf_filter.hip) are compared with.  Pass by pass, leaf by
// leaf: the leaf's 8 x 8 x (8 + 2W) values along the pass's axis, the two neighbour leaves found by bisection in the sorted list;
// the passes alternate between the caller's array and one scratch array of the same size, so that the last one writes the caller's.
// Arithmetic: float, no contraction (x86-64 has none without -mfma; the builds state -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "leaf_list.h"

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

}  // namespace

extern "C" {

int fluid_sdf_filter(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, float* values)
{
    if (check_list(g) != FLUID_OK || !f) return FLUID_ERR_ARG;
    if (f->width < 1 || f->width > 4 || f->iterations < 0 || f->iterations > 16 || !std::isfinite(f->offset) || !std::isfinite((float)f->offset))
        return FLUID_ERR_ARG;
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

}  // extern "C"
