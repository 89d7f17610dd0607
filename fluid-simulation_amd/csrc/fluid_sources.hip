// Particle sources and sinks of the one-GPU step (include/fluid_hip.h, "particle sources and sinks"): the reference's
// commented-out emitter (fluid.cc:1374-1375, 1379-1382, 1495-1497) behind the C ABI, and persistent sources / sinks that
// fluid_step applies after FLIPadvect.  Kernels in kernels_sources.hip.
#include "sim.h"
#include <algorithm>

using namespace fl;
#define fail fluid_fail

static uint64_t sm64_host(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define SRC_GUARD(s)                                                                                                     \
    if (!(s)) return fail(FLUID_ERR_ARG, "null handle");                                                                 \
    if ((s)->dist) return fail(FLUID_ERR_STATE, "these entry points are single-GPU only (they renumber the pids): a decomposed handle uses fluid_dist_set_source, fluid_dist_set_sink, fluid_dist_get_source_stats, fluid_dist_add_particles")

// a box of the index space [0, N-1]^3, not empty
static bool box_from(const fluid_sim* s, const int32_t lo[3], const int32_t hi[3], Box& b)
{
    const int N = s->g.N;
    for (int a = 0; a < 3; ++a)
        if (lo[a] < 0 || hi[a] > N - 1 || lo[a] > hi[a]) return false;
    b = Box{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    return true;
}

// block sums of launch_exclusive_scan for any count up to INT32_MAX (one allocation, made when the first slot is set)
static int ensure_sums(fluid_sim* s)
{
    if (s->src_sums) return FLUID_OK;
    HIPCHK(hipMalloc((void**)&s->src_sums, ((size_t)INT32_MAX / 2048 + 16) * sizeof(int)));
    return FLUID_OK;
}

void fl::sources_free(fluid_sim* s)
{
    for (auto& q : s->src) {
        if (q.buf) hipFree(q.buf);
        q.buf = nullptr;
    }
    if (s->src_sums) hipFree(s->src_sums);
    s->src_sums = nullptr;
}

static int read_small(fluid_sim* s, int i)
{
    HIPCHK(hipMemcpyAsync(s->h_small + i, s->d_small + i, sizeof(int), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    return FLUID_OK;
}

// every particle whose base cell lies in a sink box goes; the others keep their order (device and pid) and get pids 0..np'-1
static int apply_sinks(fluid_sim* s, long* removed)
{
    *removed = 0;
    SinkSet sk{};
    for (int i = 0; i < FLUID_MAX_SINKS; ++i)
        if (s->sink_on[i]) sk.box[sk.n++] = s->sink[i];
    if (sk.n == 0 || s->np == 0) return FLUID_OK;
    const long n = s->np;
    const Particles a = s->pa.shifted(s->p_off);
    // the count alone first (positions only: nothing else is read or written in a step where nothing goes)
    HIPCHK(hipMemsetAsync(s->d_small, 0, sizeof(int), s->st));
    launch_sink_mark(s->st, s->g, n, a, sk, nullptr, nullptr, s->d_small);
    HIPCHK(hipGetLastError());
    int rc = read_small(s, 0);
    if (rc) return rc;
    const long r = s->h_small[0];
    if (r == 0) return FLUID_OK;
    // keep flags in device order (key) and pid order (order), their scans: particle-sized scratch that holds nothing between steps
    launch_sink_mark(s->st, s->g, n, a, sk, s->key, s->order, nullptr);
    launch_exclusive_scan(s->st, s->key, s->slot, n, s->src_sums, s->d_small + 2);
    launch_exclusive_scan(s->st, s->order, s->order2, n, s->src_sums, s->d_small + 3);
    launch_sink_compact(s->st, n, a, s->pb, s->key, s->slot, s->order2);
    HIPCHK(hipGetLastError());
    std::swap(s->pa, s->pb);
    s->p_off = 0;
    s->np = n - r;
    *removed = r;
    return FLUID_OK;
}

// source slot q at step t: returns the number of points it appended
static int apply_source(fluid_sim* s, fluid_sim::SrcSlot& q, long t, long* emitted)
{
    *emitted = 0;
    const fluid_source_t& c = q.src;
    const Box b = q.box;
    const long B = b.cells();
    int *hist = q.buf, *cnt = q.buf + B, *off = q.buf + 2 * B;
    const bool fill = c.mode == FLUID_SOURCE_FILL;
    const uint64_t h0 = sm64_host(sm64_host(c.seed) ^ (uint64_t)t);
    if (fill) {
        HIPCHK(hipMemsetAsync(hist, 0, B * sizeof(int), s->st));
        launch_src_count(s->st, s->g, s->np, s->pa.shifted(s->p_off), b, hist);
    }
    launch_src_plan(s->st, s->g, b, h0, c.per_cell, fill, s->solid, hist, cnt);
    launch_exclusive_scan(s->st, cnt, off, B, s->src_sums, s->d_small + 1);
    HIPCHK(hipGetLastError());
    int rc = read_small(s, 1);
    if (rc) return rc;
    const long m = s->h_small[1];
    if (m == 0) return FLUID_OK;
    if (s->np + m > (long)INT32_MAX) return fail(FLUID_ERR_STATE, "a source would take the particle count past INT32_MAX");
    if ((rc = grow_particles(s, s->p_off + s->np + m))) return rc;
    const Particles p = s->pa.shifted(s->p_off + s->np);
    const double zero[3] = {0, 0, 0};
    launch_src_emit(s->st, s->g, b, h0, c.per_cell, fill, s->solid, hist, off, p, (uint32_t)s->np, c.vel_mode == FLUID_SOURCE_VEL_FIXED ? c.vel : zero);
    if (c.vel_mode == FLUID_SOURCE_VEL_GRID) launch_interp_from_grid(s->st, s->g, m, p, s->u, s->v, s->w);
    HIPCHK(hipGetLastError());
    s->np += m;
    *emitted = m;
    return FLUID_OK;
}

// After FLIPadvect (fluid.cc:1495-1497): the sinks, then the sources in slot order.  The grid still holds this step's
// velocities after the update (the next step's P2G clears them).
int fl::sources_apply(fluid_sim* s)
{
    s->src_emit_last = s->src_rm_last = 0;
    bool any = false;
    for (int i = 0; i < FLUID_MAX_SINKS; ++i) any = any || s->sink_on[i];
    for (const auto& q : s->src) any = any || q.on;
    if (!any) return FLUID_OK;
    s->binned = false;   // the sinks use key / slot as scratch, both change the particle set: the next sort bins for itself
    const long t = s->n_steps;
    long removed = 0, emitted = 0;
    int rc = apply_sinks(s, &removed);
    if (rc) return rc;
    for (auto& q : s->src) {
        if (!q.on || t % q.src.every != 0) continue;
        long m = 0;
        if ((rc = apply_source(s, q, t, &m))) return rc;
        emitted += m;
        if (m > 0 && !box_empty(s->Pb)) {   // the next sort's x-plane guess (Pb +- 3) covers the new points: their base cells lie in q.box
            Box& P = s->Pb;
            P = Box{std::min(P.x0, q.box.x0), std::min(P.y0, q.box.y0), std::min(P.z0, q.box.z0),
                    std::max(P.x1, q.box.x1), std::max(P.y1, q.box.y1), std::max(P.z1, q.box.z1)};
        }
    }
    s->src_emit_last = emitted, s->src_rm_last = removed;
    s->src_emit_total += emitted, s->src_rm_total += removed;
    if (emitted || removed) s->stats.paths |= FLUID_PATH_SOURCES;
    return FLUID_OK;
}

extern "C" {

int fluid_add_particles(fluid_sim_t* s, int64_t n, const double* pos, const double* vel)
{
    SRC_GUARD(s);
    if (n < 0 || (n > 0 && !pos)) return fail(FLUID_ERR_ARG, "bad particle arguments");
    if (!vel && !s->vel_ok) return fail(FLUID_ERR_STATE, "add_particles with vel == NULL needs the grid velocities of a completed step");
    if (s->np + (long)n > (long)INT32_MAX) return fail(FLUID_ERR_STATE, "more than INT32_MAX particles");
    if (n == 0) return FLUID_OK;
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = grow_particles(s, s->p_off + s->np + (long)n);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(s->stage_pos, pos, 3 * n * sizeof(double), hipMemcpyHostToDevice, s->st));
    if (vel) HIPCHK(hipMemcpyAsync(s->stage_vel, vel, 3 * n * sizeof(double), hipMemcpyHostToDevice, s->st));
    const Particles p = s->pa.shifted(s->p_off + s->np);
    launch_src_append(s->st, (long)n, s->stage_pos, vel ? s->stage_vel : nullptr, p, (uint32_t)s->np);
    if (!vel) launch_interp_from_grid(s->st, s->g, (long)n, p, s->u, s->v, s->w);   // PointList::interpFromGrid, fluid.cc:883-894
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->st));
    s->np += (long)n;
    s->sorted = s->have_p2g = s->have_flags = false;
    s->sort_hint = false;   // (the warm start, have_guess, stays: the same scene a little fuller)
    s->binned = false;
    return FLUID_OK;
}

int fluid_set_source(fluid_sim_t* s, int32_t slot, const fluid_source_t* src)
{
    SRC_GUARD(s);
    if (slot < 0 || slot >= FLUID_MAX_SOURCES) return fail(FLUID_ERR_ARG, "source slot out of range");
    auto& q = s->src[slot];
    HIPCHK(hipSetDevice(s->prm.device));
    if (!src) {
        HIPCHK(hipStreamSynchronize(s->st));
        if (q.buf) hipFree(q.buf);
        q = fluid_sim::SrcSlot{};
        return FLUID_OK;
    }
    Box b;
    if (!box_from(s, src->lo, src->hi, b)) return fail(FLUID_ERR_ARG, "source box empty or off the grid");
    if (src->per_cell < 1 || src->per_cell > 64) return fail(FLUID_ERR_ARG, "per_cell must be in 1..64");
    if (src->mode != FLUID_SOURCE_ADD && src->mode != FLUID_SOURCE_FILL) return fail(FLUID_ERR_ARG, "bad source mode");
    if (src->vel_mode != FLUID_SOURCE_VEL_FIXED && src->vel_mode != FLUID_SOURCE_VEL_GRID) return fail(FLUID_ERR_ARG, "bad source vel_mode");
    if (src->every < 1) return fail(FLUID_ERR_ARG, "every must be >= 1");
    if ((double)b.cells() * src->per_cell > (double)INT32_MAX) return fail(FLUID_ERR_ARG, "source box x per_cell exceeds INT32_MAX points");
    int rc = ensure_sums(s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s->st));
    if (q.buf) hipFree(q.buf);
    q.buf = nullptr;
    q.on = false;
    HIPCHK(hipMalloc((void**)&q.buf, 3 * (size_t)b.cells() * sizeof(int)));
    q.src = *src;
    q.box = b;
    q.on = true;
    return FLUID_OK;
}

int fluid_set_sink(fluid_sim_t* s, int32_t slot, const int32_t lo[3], const int32_t hi[3])
{
    SRC_GUARD(s);
    if (slot < 0 || slot >= FLUID_MAX_SINKS) return fail(FLUID_ERR_ARG, "sink slot out of range");
    if (!lo) {
        s->sink_on[slot] = false;
        return FLUID_OK;
    }
    Box b;
    if (!hi || !box_from(s, lo, hi, b)) return fail(FLUID_ERR_ARG, "sink box empty or off the grid");
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = ensure_sums(s);
    if (rc) return rc;
    s->sink[slot] = b;
    s->sink_on[slot] = true;
    return FLUID_OK;
}

int fluid_get_source_stats(fluid_sim_t* s, int64_t* emitted_last, int64_t* removed_last, int64_t* emitted_total, int64_t* removed_total)
{
    SRC_GUARD(s);
    if (emitted_last) *emitted_last = s->src_emit_last;
    if (removed_last) *removed_last = s->src_rm_last;
    if (emitted_total) *emitted_total = s->src_emit_total;
    if (removed_total) *removed_total = s->src_rm_total;
    return FLUID_OK;
}

}  // extern "C"
