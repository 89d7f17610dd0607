// fluid_particles_trails and fluid_spheres_surface (include/fluid_hip.h, "liquid surface, velocity trails"): the expansion of
// particles into instances and the dense level set of (position, radius) items on the host, with the arithmetic of sdf_trail_def.h
// that the kernels use (kernels_sdf_trail.hip).  No leaves, no device: the counted items are binned by base cell (a counting sort,
// z fastest), and every voxel of the grid looks at every item of every cell within 4 cells of it.  An OR and a minimum do not care
// in which order.  Built with -ffp-contract=off (Makefile).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fluid_hip.h"
#include "sdf_trail_def.h"

namespace {

bool params_ok(const fluid_sdf_params_t* p)
{
    if (!p) return false;
    const float R = (float)p->radius, w = (float)p->half_width;
    const float mx = R + w;
    return p->radius > 0 && R > 0.0f && w >= 1.0f && mx <= 4.0f;
}

}  // namespace

extern "C" int64_t fluid_particles_trails(int64_t np, const double* pos, const double* vel, const fluid_sdf_params_t* p,
                                          const fluid_sdf_trails_t* t, int64_t cap, double* out_pos, float* out_radius)
{
    const bool count_only = !out_pos && !out_radius;
    if (np < 0 || (np > 0 && !pos) || !params_ok(p) || !t || (!count_only && (!out_pos || !out_radius))) return -FLUID_ERR_ARG;
    if (!tdef::settings_ok(t->shutter, t->delta, t->radius_min, t->max_instances, t->reserved)) return -FLUID_ERR_ARG;
    const float R = (float)p->radius;
    if (!tdef::radius_ok(t->radius_min, R)) return -FLUID_ERR_ARG;
    const tdef::Consts tc = tdef::consts(t->shutter, t->delta, t->radius_min, t->max_instances, R);
    // two passes: a refusal must write nothing
    int64_t count = 0;
    for (int pass = 0; pass < (count_only ? 1 : 2); ++pass) {
        if (pass == 1 && count > cap) return -FLUID_ERR_ARG;
        count = 0;
        for (int64_t i = 0; i < np; ++i) {
            const double* q = pos + 3 * i;
            tdef::Trail T = vel ? tdef::trail(tc, vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]) : tdef::trail(tc, 0.0, 0.0, 0.0);
            int k = 0;
            do {
                if (pass == 1) {
                    for (int a = 0; a < 3; ++a) out_pos[3 * count + a] = tdef::at(T, q[a], a);
                    out_radius[count] = T.r;
                }
                ++count, ++k;
            } while (k < tdef::MAX_INSTANCES && tdef::next(tc, T));
        }
    }
    return count;
}

extern "C" int fluid_spheres_surface(int32_t n, double dx, int64_t n_items, const double* pos, const float* radius, const fluid_sdf_params_t* p,
                                     float* values, uint8_t* active)
{
    if (n < 1 || !(dx > 0) || n_items < 0 || (n_items > 0 && (!pos || !radius)) || !params_ok(p) || !values) return FLUID_ERR_ARG;
    const float R = (float)p->radius, w = (float)p->half_width, dxf = (float)dx;
    const float bg = dxf * w;
    for (int64_t i = 0; i < n_items; ++i)
        if (!(radius[i] > 0.0f && radius[i] <= R)) return FLUID_ERR_ARG;
    const int lo = -(n / 2), hi = lo + n - 1;
    const size_t nc = (size_t)n * n * n;

    // the counted items in cell order
    auto cell_of = [&](const double* q, size_t& c) {
        const double rx = std::round(q[0]), ry = std::round(q[1]), rz = std::round(q[2]);
        if (!(rx >= (double)lo && rx <= (double)hi && ry >= (double)lo && ry <= (double)hi && rz >= (double)lo && rz <= (double)hi)) return false;
        c = ((size_t)((int)rx - lo) * n + (size_t)((int)ry - lo)) * n + (size_t)((int)rz - lo);
        return true;
    };
    std::vector<int64_t> first(nc + 1, 0);
    for (int64_t i = 0; i < n_items; ++i) {
        size_t c;
        if (cell_of(pos + 3 * i, c)) ++first[c + 1];
    }
    for (size_t c = 0; c < nc; ++c) first[c + 1] += first[c];
    std::vector<double> sorted((size_t)first[nc] * 3);
    std::vector<tdef::Ball> balls((size_t)first[nc]);
    {
        std::vector<int64_t> next(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < n_items; ++i) {
            size_t c;
            if (!cell_of(pos + 3 * i, c)) continue;
            const size_t d = (size_t)next[c]++;
            sorted[3 * d] = pos[3 * i], sorted[3 * d + 1] = pos[3 * i + 1], sorted[3 * d + 2] = pos[3 * i + 2];
            balls[d] = tdef::ball(radius[i], w);
        }
    }

    const int K = 4;   // r <= R and R + w <= 4: no item further out than ring 4 reaches the voxel
    for (int vx = lo; vx <= hi; ++vx)
        for (int vy = lo; vy <= hi; ++vy)
            for (int vz = lo; vz <= hi; ++vz) {
                bool inside = false;
                float d = INFINITY;
                const int z0 = std::max(vz - K, lo), z1 = std::min(vz + K, hi);
                for (int cx = std::max(vx - K, lo); cx <= std::min(vx + K, hi); ++cx)
                    for (int cy = std::max(vy - K, lo); cy <= std::min(vy + K, hi); ++cy) {
                        const size_t row = ((size_t)(cx - lo) * n + (size_t)(cy - lo)) * n;
                        // the cells of a z run are one range of the sorted array
                        for (int64_t i = first[row + (size_t)(z0 - lo)]; i < first[row + (size_t)(z1 - lo) + 1]; ++i) {
                            const double* q = &sorted[(size_t)i * 3];
                            const tdef::Ball& b = balls[(size_t)i];
                            tdef::visit(inside, d, tdef::dist2(vx, vy, vz, q[0], q[1], q[2]), b.r, b.max2, b.min2, dxf);
                        }
                    }
                const size_t c = ((size_t)(vx - lo) * n + (size_t)(vy - lo)) * n + (size_t)(vz - lo);
                bool act;
                tdef::finish(inside, d, bg, values[c], act);
                if (active) active[c] = act ? 1 : 0;
            }
    return FLUID_OK;
}
