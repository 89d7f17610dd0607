// The plan of the level-set filter (include/fluid_hip.h, "liquid surface, smoothed", "renormalised", "grown band", "flows"), stated
// once for the device's front half (fluid_sdf.hip, hipcc) and the host functions (sdf_filter_host.cpp, g++): which arguments are
// taken, how many tracks a filter runs, and the order of its passes (box or flow), offset steps and tracks.  Host code only.  What
// a pass, an offset and a track consist of is each side's own: launches there, loops over a leaf list here.  The callers keep
// their error texts.
#pragma once
#include <cmath>

#include "../../include/fluid_hip.h"
#include "sdf_track_def.h"

namespace plan {

// ---- the argument rules -----------------------------------------------------------------------------------------------------------
inline bool filter_ok(const fluid_sdf_filter_t* f)
{
    return f && f->width >= 1 && f->width <= 4 && f->iterations >= 0 && f->iterations <= 16 && std::isfinite(f->offset) && std::isfinite((float)f->offset);
}
// the filter's kind ("liquid surface, flows") and the width it admits beside filter_ok: the median's cube is 27 or 125 values, the
// Laplacian and the mean-curvature stencil have one width
inline bool kind_ok(int kind) { return kind >= FLUID_SDF_FILTER_BOX && kind <= FLUID_SDF_FILTER_MEAN_CURVATURE; }
inline bool width_ok(int kind, int W) { return kind == FLUID_SDF_FILTER_BOX ? true : kind == FLUID_SDF_FILTER_MEDIAN ? W <= 2 : W == 1; }
// does a pass of the kind read dx?  (an untracked box or median filter does not)
inline bool kind_needs_dx(int kind) { return kind == FLUID_SDF_FILTER_LAPLACIAN || kind == FLUID_SDF_FILTER_MEAN_CURVATURE; }
// (a null track: tracking off)
inline bool track_ok(const fluid_sdf_track_t* t)
{
    return !t || (t->normalize >= 0 && t->normalize <= tdef::MAX_PASSES && (t->trim == 0 || t->trim == 1) &&
                  (t->scheme == FLUID_SDF_TRACK_FIRST_BIAS || t->scheme == FLUID_SDF_TRACK_HJWENO5));
}
inline bool tracking(const fluid_sdf_track_t* t) { return t && (t->normalize > 0 || t->trim != 0); }
// growing the band: every track normalises and trims
inline bool grow_ok(const fluid_sdf_track_t* t) { return t && t->normalize >= 1 && t->trim == 1; }
// the offset of a tracked filter stays within the band, that of a grown one within 4 dx
inline bool tracked_offset_ok(float off, float bg) { return !(std::fabs(off) > bg); }
inline bool grown_offset_ok(float off, float dx) { return !(std::fabs(off) > 4.0f * dx); }

// ---- the schedule -----------------------------------------------------------------------------------------------------------------
// A tracked offset is taken in steps of at most dx / 2 (tdef::offset_step): step(signed size) for each, in order; returns how many.
template <typename Step> inline int offset_steps(float off, float dx, Step step)
{
    const float a = std::fabs(off);
    float d = 0.0f;
    int n = 0;
    for (float delta; (delta = tdef::offset_step(a, d, dx)) != 0.0f; ++n) {
        d = d + delta;
        step(std::copysign(delta, off));
    }
    return n;
}
// T: the tracks a tracked filter runs, one per iteration and per offset step
inline int tracks(const fluid_sdf_filter_t& f, float dx) { return f.iterations + offset_steps((float)f.offset, dx, [](float) {}); }

// the passes of one iteration: the box filter's three axes, one pass of a flow
inline int iteration_passes(int kind) { return kind == FLUID_SDF_FILTER_BOX ? 3 : 1; }
inline int passes(int kind, const fluid_sdf_filter_t& f) { return iteration_passes(kind) * f.iterations; }

// The filter: `iterations` times the passes of its kind: the box passes box(axis, width, offset added to the pass's results) in the
// library's order x, z, y, or the one pass flow(kind, width, offset added likewise) of a median, Laplacian or mean-curvature flow.
// Tracked: track() after every iteration, then the offset in steps, offset(step) and track() for each.  Untracked: the offset rides
// on the last pass, or is an offset(off) of its own when there is no pass; here dx is not read.
template <typename Box, typename Flow, typename Offset, typename Track>
inline void run(int kind, const fluid_sdf_filter_t& f, float dx, bool tracked, Box box, Flow flow, Offset offset, Track track)
{
    static const int axes[3] = {0, 2, 1};
    const int per = iteration_passes(kind), passes = per * f.iterations;
    const float off = (float)f.offset;
    for (int k = 0; k < passes; ++k) {
        const float ride = !tracked && k == passes - 1 ? off : 0.0f;
        if (kind == FLUID_SDF_FILTER_BOX) box(axes[k % 3], f.width, ride);
        else flow(kind, f.width, ride);
        if (tracked && k % per == per - 1) track();
    }
    if (tracked) offset_steps(off, dx, [&](float step) { offset(step), track(); });
    else if (passes == 0 && off != 0.0f) offset(off);
}

}  // namespace plan
