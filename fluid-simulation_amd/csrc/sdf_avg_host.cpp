// fluid_particles_surface (include/fluid_hip.h, "liquid surface, averaged positions"): the dense level set of a particle set on the
// host, for the spheres and for the averaged positions, with the arithmetic of sdf_avg_def.h that the kernel uses
// (kernels_sdf_avg.hip).  No leaves, no rings with stops, no device: the counted particles are binned by base cell (a counting
// sort, z fastest), and every voxel of the grid looks at every particle of every cell within adef::LAST_RING cells of it.  A
// minimum and wrapping integer sums do not care in which order.  Built with -ffp-contract=off (Makefile).
//
// fluid_sdf_avg_grids_merge ("liquid surface, averaged positions (decomposed runs)"): the ranks' records of (dist2, SW, SX, SY, SZ)
// into the leaf list of the union, by the cursor walk of leaf_list.h and adef::finish.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fluid_hip.h"
#include "leaf_list.h"
#include "sdf_avg_def.h"

extern "C" int fluid_particles_surface(int32_t n, double dx, int64_t np, const double* pos, const fluid_sdf_params_t* p,
                                       const fluid_sdf_surface_t* sf, float* values, uint8_t* active)
{
    if (n < 1 || !(dx > 0) || np < 0 || (np > 0 && !pos) || !p || !values) return FLUID_ERR_ARG;
    const float R = (float)p->radius, w = (float)p->half_width, dxf = (float)dx;
    const float mx = R + w;
    if (!(p->radius > 0) || !(R > 0.0f) || !(w >= 1.0f) || !(mx <= 4.0f)) return FLUID_ERR_ARG;
    const bool averaged = sf && sf->kind != FLUID_SDF_SURFACE_SPHERES;
    if (averaged && (sf->kind != FLUID_SDF_SURFACE_AVERAGED || sf->reserved != 0 || !adef::influence_ok(sf->influence))) return FLUID_ERR_ARG;
    const adef::Consts hc = averaged ? adef::consts(sf->influence) : adef::Consts{0.0f, 0.0f};
    const float bg = dxf * w, max2 = mx * mx;
    const float mn = std::fmax(0.0f, R - w);
    const float min2 = mn * mn;
    const int lo = -(n / 2), hi = lo + n - 1;
    const size_t nc = (size_t)n * n * n;

    // the counted particles in cell order
    auto cell_of = [&](const double* q, size_t& c) {
        const double rx = std::round(q[0]), ry = std::round(q[1]), rz = std::round(q[2]);
        if (!(rx >= (double)lo && rx <= (double)hi && ry >= (double)lo && ry <= (double)hi && rz >= (double)lo && rz <= (double)hi)) return false;
        c = ((size_t)((int)rx - lo) * n + (size_t)((int)ry - lo)) * n + (size_t)((int)rz - lo);
        return true;
    };
    std::vector<int64_t> first(nc + 1, 0);
    for (int64_t i = 0; i < np; ++i) {
        size_t c;
        if (cell_of(pos + 3 * i, c)) ++first[c + 1];
    }
    for (size_t c = 0; c < nc; ++c) first[c + 1] += first[c];
    std::vector<double> sorted((size_t)first[nc] * 3);
    {
        std::vector<int64_t> next(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < np; ++i) {
            size_t c;
            if (!cell_of(pos + 3 * i, c)) continue;
            double* d = &sorted[(size_t)next[c]++ * 3];
            d[0] = pos[3 * i], d[1] = pos[3 * i + 1], d[2] = pos[3 * i + 2];
        }
    }

    const int K = adef::LAST_RING;
    for (int vx = lo; vx <= hi; ++vx)
        for (int vy = lo; vy <= hi; ++vy)
            for (int vz = lo; vz <= hi; ++vz) {
                float m = INFINITY;
                adef::Sums sum;
                const int z0 = std::max(vz - K, lo), z1 = std::min(vz + K, hi);
                for (int cx = std::max(vx - K, lo); cx <= std::min(vx + K, hi); ++cx)
                    for (int cy = std::max(vy - K, lo); cy <= std::min(vy + K, hi); ++cy) {
                        const size_t row = ((size_t)(cx - lo) * n + (size_t)(cy - lo)) * n;
                        // the cells of a z run are one range of the sorted array
                        for (int64_t i = first[row + (size_t)(z0 - lo)]; i < first[row + (size_t)(z1 - lo) + 1]; ++i) {
                            const double* q = &sorted[(size_t)i * 3];
                            const float x2 = adef::dist2(vx, vy, vz, q[0], q[1], q[2]);
                            m = std::fmin(m, x2);
                            if (averaged && x2 < hc.h2)
                                adef::add(sum, adef::weight(x2, hc), adef::offset(q[0], vx), adef::offset(q[1], vy), adef::offset(q[2], vz));
                        }
                    }
                const size_t c = ((size_t)(vx - lo) * n + (size_t)(vy - lo)) * n + (size_t)(vz - lo);
                bool act;
                adef::finish(m, sum, averaged, R, dxf, bg, max2, min2, values[c], act);
                if (active) active[c] = act ? 1 : 0;
            }
    return FLUID_OK;
}

namespace {

inline uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// what fluid_sdf_avg_grids_merge refuses in its parts
bool avg_parts_merge(const fluid_sdf_avg_part_t* parts, int32_t n_parts)
{
    const fluid_sdf_avg_part_t& a = parts[0];
    const float mx = a.radius + a.half_width;
    if (!(a.radius > 0.0f) || !(a.half_width >= 1.0f) || !(mx <= 4.0f) || !(a.dx > 0.0f) || !adef::influence_ok((double)a.influence) ||
        bits_of(a.background) != bits_of(a.dx * a.half_width))
        return false;
    for (int p = 0; p < n_parts; ++p) {
        const fluid_sdf_avg_part_t& g = parts[p];
        if (g.n != a.n || bits_of(g.background) != bits_of(a.background) || bits_of(g.radius) != bits_of(a.radius) ||
            bits_of(g.half_width) != bits_of(a.half_width) || bits_of(g.dx) != bits_of(a.dx) || bits_of(g.influence) != bits_of(a.influence))
            return false;
        if (check_origins(&g, g.origin && g.dist2 && g.sums) != FLUID_OK) return false;
        for (size_t l = 0; l < (size_t)g.n_leaves; ++l)
            for (int v = 0; v < 512; ++v) {
                const float d = g.dist2[512 * l + v];
                if (std::isnan(d) || std::signbit(d)) return false;
                if (d == 0.0f || std::isinf(d))
                    for (int k = 0; k < 4; ++k)
                        if (g.sums[(4 * l + k) * 512 + v] != 0) return false;
            }
    }
    return true;
}

}  // namespace

// Two passes over the walk, each computing a merged leaf into buffers of one leaf: the first counts the leaves that hold anything
// but inactive +bg (a refusal must write nothing), the second copies them into the caller's arrays.
extern "C" int64_t fluid_sdf_avg_grids_merge(const fluid_sdf_avg_part_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin,
                                             float* values, uint64_t* active)
{
    const bool count_only = !origin && !values && !active;
    if (!parts || n_parts < 1 || (!count_only && (!origin || !values || !active))) return -FLUID_ERR_ARG;
    if (!avg_parts_merge(parts, n_parts)) return -FLUID_ERR_ARG;
    const float R = parts[0].radius, w = parts[0].half_width, dxf = parts[0].dx, bg = parts[0].background;
    const float mx = R + w, max2 = mx * mx;
    const float mn = std::fmax(0.0f, R - w);
    const float min2 = mn * mn;
    auto n_leaves_of = [&](int p) { return parts[p].n_leaves; };
    auto origin_of = [&](int p, long l) { return org_of(&parts[p], l); };
    float val[512];
    uint64_t words[8];
    int64_t count = 0;
    for (int pass = 0; pass < (count_only ? 1 : 2); ++pass) {
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        count = 0;
        merge_walk(n_parts, n_leaves_of, origin_of, [&](const Org& o, int n_in, const int32_t* part, const int32_t* leaf) {
            bool listed = false;
            memset(words, 0, sizeof words);
            for (int v = 0; v < 512; ++v) {
                float m = INFINITY;
                adef::Sums sum;
                for (int t = 0; t < n_in; ++t) {
                    const fluid_sdf_avg_part_t& g = parts[part[t]];
                    const size_t l = (size_t)leaf[t];
                    m = std::fmin(m, g.dist2[512 * l + v]);
                    const uint64_t* q = g.sums + 2048 * l + v;
                    sum.w += q[0], sum.x += q[512], sum.y += q[1024], sum.z += q[1536];
                }
                bool act;
                adef::finish(m, sum, true, R, dxf, bg, max2, min2, val[v], act);   // a voxel outside the grid has +inf on every part: +bg
                if (act) words[v >> 6] |= 1ull << (v & 63);
                listed = listed || act || val[v] != bg;
            }
            if (!listed) return true;
            if (pass == 1) {
                memcpy(values + 512 * (size_t)count, val, sizeof val);
                memcpy(active + 8 * (size_t)count, words, sizeof words);
                memcpy(origin + 3 * (size_t)count, &o, sizeof o);
            }
            count++;
            return true;
        });
    }
    return count;
}
