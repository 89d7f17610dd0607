// The plan of the level-set filter (include/fluid_hip.h, "liquid surface, smoothed", "renormalised", "grown band"), stated once for
// the device's front half (fluid_sdf.hip, hipcc) and the host functions (sdf_filter_host.cpp, g++): which arguments are taken, how
// many tracks a filter runs, and the order of its box passes, offset steps and tracks.  Host code only.  What a box pass, an offset
// and a track consist of is each side's own: launches there, loops over a leaf list here.  The callers keep their error texts.
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
// (a null track: tracking off)
inline bool track_ok(const fluid_sdf_track_t* t)
{
    return !t || (t->normalize >= 0 && t->normalize <= tdef::MAX_PASSES && (t->trim == 0 || t->trim == 1) && t->scheme == FLUID_SDF_TRACK_FIRST_BIAS);
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

// The filter: `iterations` times the box passes box(axis, width, offset added to the pass's results) in the library's order x, z, y.
// Tracked: track() after every iteration, then the offset in steps, offset(step) and track() for each.  Untracked: the offset rides
// on the last pass, or is an offset(off) of its own when there is no pass; dx is not read.
template <typename Box, typename Offset, typename Track>
inline void run(const fluid_sdf_filter_t& f, float dx, bool tracked, Box box, Offset offset, Track track)
{
    static const int axes[3] = {0, 2, 1};
    const int passes = 3 * f.iterations;
    const float off = (float)f.offset;
    for (int k = 0; k < passes; ++k) {
        box(axes[k % 3], f.width, !tracked && k == passes - 1 ? off : 0.0f);
        if (tracked && k % 3 == 2) track();
    }
    if (tracked) offset_steps(off, dx, [&](float step) { offset(step), track(); });
    else if (passes == 0 && off != 0.0f) offset(off);
}

}  // namespace plan
