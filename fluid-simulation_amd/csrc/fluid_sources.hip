// Particle sources and sinks (include/fluid_hip.h, "particle sources and sinks"): the reference's commented-out emitter
// (fluid.cc:1374-1375, 1379-1382, 1495-1497) behind the C ABI, and persistent sources / sinks that fluid_step applies after
// FLIPadvect.  The slots, the helpers and the bodies of the entry points serve both kinds of handle; the one-GPU step
// (sources_apply) is here, the collective skeleton of a decomposed step (dist_sources_apply) in fluid_dist.hip.  Kernels in
// kernels_sources.hip.
#include "sim.h"
#include <algorithm>

using namespace fl;
#define fail fluid_fail

// the two kinds of handle: what the other kind's entry points say (the guards of the wrappers here and in fluid_dist.hip)
const char* const fl::SRC_SINGLE = "these entry points are single-GPU only (they renumber the pids): a decomposed handle uses fluid_dist_set_source, fluid_dist_set_sink, fluid_dist_get_source_stats, fluid_dist_add_particles";
const char* const fl::SRC_DIST = "not a decomposed handle: a fluid_create handle uses the one-GPU entry points (fluid_set_source, fluid_set_sink, fluid_get_source_stats, fluid_add_particles)";

// a box of the index space [0, N-1]^3, not empty
static bool index_box(const fluid_sim* s, const int32_t lo[3], const int32_t hi[3], Box& b)
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

// One GPU: 3 int arrays.  Decomposed: 5, then the global solid bytes of the box (a window holds only a part of the box, and
// every rank counts the kept points of ALL its cells)
static size_t slot_bytes(const fluid_sim* s, const Box& b)
{
    const size_t B = (size_t)b.cells();
    return s->dist ? 5 * B * sizeof(int) + B + 16 : 3 * B * sizeof(int);
}
SrcBuf fl::source_buf(const fluid_sim* s, const fluid_sim::SrcSlot& q)
{
    const long B = q.box.cells();
    int* b = q.buf;
    if (!s->dist) return SrcBuf{b, b + B, b + 2 * B, nullptr, b + 2 * B, nullptr};
    return SrcBuf{b, b + B, b + 2 * B, b + 3 * B, b + 4 * B, (uint8_t*)(b + 5 * B)};
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

// re-balance: the slots (their buffers are box-sized, global: nothing in them belongs to the old window), the sinks, the scans'
// block sums and the four counters go to the new window's handle; n_steps, the t of the sources, goes with output_move
void fl::sources_move(fluid_sim* from, fluid_sim* to)
{
    for (int i = 0; i < FLUID_MAX_SOURCES; ++i) std::swap(to->src[i], from->src[i]);
    for (int i = 0; i < FLUID_MAX_SINKS; ++i) { to->sink[i] = from->sink[i]; to->sink_on[i] = from->sink_on[i]; }
    std::swap(to->src_sums, from->src_sums);
    to->src_emit_last = from->src_emit_last, to->src_rm_last = from->src_rm_last;
    to->src_emit_total = from->src_emit_total, to->src_rm_total = from->src_rm_total;
}

SinkSet fl::sinks_on(const fluid_sim* s)
{
    SinkSet sk{};
    for (int i = 0; i < FLUID_MAX_SINKS; ++i)
        if (s->sink_on[i]) sk.box[sk.n++] = s->sink[i];
    return sk;
}

// ---- a due source, in the halves that a decomposed step puts its collectives between ------------------------------------------
// slot q at step t on a handle that owns the cells of ob
SrcDue fl::source_due(const fluid_sim* s, const fluid_sim::SrcSlot& q, long t, const OwnBox& ob)
{
    const Box& b = q.box;
    const long N = s->g.N;
    SrcDue u{&q, source_buf(s, q), sm64(sm64(q.src.seed) ^ (uint64_t)t), q.src.mode == FLUID_SOURCE_FILL, ob, {}};
    if (s->dist) u.sv = SolidView{u.a.mask, {b.x0, b.y0, b.z0}, (long)b.ny() * b.nz(), b.nz()};
    else u.sv = SolidView{s->solid, {0, 0, 0}, N * N, N};
    if (ob.lo[0] <= b.x0 && b.x1 < ob.hi[0] && ob.lo[1] <= b.y0 && b.y1 < ob.hi[1] && ob.lo[2] <= b.z0 && b.z1 < ob.hi[2])
        u.a.cnt_own = nullptr, u.a.off_own = u.a.off;   // the whole box is this handle's: one scan places and numbers
    return u;
}

// FILL: this handle's live particles per cell of the box (enqueued; a decomposed run sums the ranks' histograms next)
int fl::source_count(fluid_sim* s, const SrcDue& u)
{
    if (!u.fill) return FLUID_OK;
    HIPCHK(hipMemsetAsync(u.a.hist, 0, u.q->box.cells() * sizeof(int), s->st));
    launch_src_count(s->st, s->g, s->np, s->pa.shifted(s->p_off), u.q->box, u.a.hist, s->dist);
    HIPCHK(hipGetLastError());
    return FLUID_OK;
}

// kept points per cell, their scans, the totals read back: *m = the new points of the whole box, *mo = this handle's
int fl::source_plan(fluid_sim* s, const SrcDue& u, long* m, long* mo)
{
    const Box& b = u.q->box;
    const long B = b.cells();
    launch_src_plan(s->st, s->g, b, u.h0, u.q->src.per_cell, u.fill, u.ob, u.sv, u.a.hist, u.a.cnt, u.a.cnt_own);
    launch_exclusive_scan(s->st, u.a.cnt, u.a.off, B, s->src_sums, s->d_small + 1);
    if (u.a.cnt_own) launch_exclusive_scan(s->st, u.a.cnt_own, u.a.off_own, B, s->src_sums, s->d_small + 2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_small + 1, s->d_small + 1, (u.a.cnt_own ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    *m = s->h_small[1];
    *mo = u.a.cnt_own ? s->h_small[2] : *m;
    return FLUID_OK;
}

// room for mo more particles behind the live ones
int fl::source_room(fluid_sim* s, long mo)
{
    if (s->np + mo > (long)INT32_MAX) return fail(FLUID_ERR_STATE, "a source would take the particle count past INT32_MAX");
    return grow_particles(s, s->p_off + s->np + mo);
}

// this handle's points into p (the arrays from the first new slot on), ids from id0 on in the box's cell order
void fl::source_emit(fluid_sim* s, const SrcDue& u, Particles p, uint32_t id0)
{
    const fluid_source_t& c = u.q->src;
    const double zero[3] = {0, 0, 0};
    launch_src_emit(s->st, s->g, u.q->box, u.h0, c.per_cell, u.fill, u.ob, u.sv, u.a.hist, u.a.off, u.a.off_own, p, id0,
                    c.vel_mode == FLUID_SOURCE_VEL_FIXED ? c.vel : zero);
}

// the next sort's x-plane guess (Pb +- 3) covers the new points of GLOBAL index box b: the part of it in this handle's window
void fl::source_widen_Pb(fluid_sim* s, const Box& b)
{
    const Grid& g = s->g;
    const Box w{std::max(b.x0 - g.ox, 0), std::max(b.y0 - g.oy, 0), std::max(b.z0 - g.oz, 0),
                std::min(b.x1 - g.ox, g.nx - 1), std::min(b.y1 - g.oy, g.ny - 1), std::min(b.z1 - g.oz, g.nz - 1)};
    Box& P = s->Pb;
    if (box_empty(w)) return;
    P = box_empty(P) ? w
                     : Box{std::min(P.x0, w.x0), std::min(P.y0, w.y0), std::min(P.z0, w.z0), std::max(P.x1, w.x1), std::max(P.y1, w.y1),
                           std::max(P.z1, w.z1)};
}

void fl::sources_tally(fluid_sim* s, long emitted, long removed)
{
    s->src_emit_last = emitted, s->src_rm_last = removed;
    s->src_emit_total += emitted, s->src_rm_total += removed;
}

static int read_small(fluid_sim* s, int i)
{
    HIPCHK(hipMemcpyAsync(s->h_small + i, s->d_small + i, sizeof(int), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    return FLUID_OK;
}

// One GPU: every particle whose base cell lies in a sink box goes; the others keep their order (device and pid) and get pids
// 0..np'-1 (a decomposed run marks them dead where they are: dist_sources_apply)
static int apply_sinks(fluid_sim* s, long* removed)
{
    *removed = 0;
    const SinkSet sk = sinks_on(s);
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

// One GPU, after FLIPadvect (fluid.cc:1495-1497): the sinks, then the sources in slot order.  The grid still holds this step's
// velocities after the update (the next step's P2G clears them).  The handle is the whole-grid window: it owns every box.
int fl::sources_apply(fluid_sim* s)
{
    s->src_emit_last = s->src_rm_last = 0;
    bool any = false;
    for (int i = 0; i < FLUID_MAX_SINKS; ++i) any = any || s->sink_on[i];
    for (const auto& q : s->src) any = any || q.on;
    if (!any) return FLUID_OK;
    s->binned = false;   // the sinks use key / slot as scratch, both change the particle set: the next sort bins for itself
    const long t = s->n_steps;
    const int N = s->g.N;
    const OwnBox all{{0, 0, 0}, {N, N, N}, {0, 0, 0}, {0, 0, 0}};
    long removed = 0, emitted = 0;
    int rc = apply_sinks(s, &removed);
    if (rc) return rc;
    for (auto& q : s->src) {
        if (!q.on || t % q.src.every != 0) continue;
        const SrcDue u = source_due(s, q, t, all);
        long m = 0, mo = 0;
        if ((rc = source_count(s, u)) || (rc = source_plan(s, u, &m, &mo))) return rc;
        if (m == 0) continue;
        if ((rc = source_room(s, m))) return rc;
        const Particles p = s->pa.shifted(s->p_off + s->np);
        source_emit(s, u, p, (uint32_t)s->np);
        if (q.src.vel_mode == FLUID_SOURCE_VEL_GRID) launch_interp_from_grid(s->st, s->g, m, p, s->u, s->v, s->w);
        HIPCHK(hipGetLastError());
        s->np += m;
        emitted += m;
        if (!box_empty(s->Pb)) source_widen_Pb(s, q.box);   // (their base cells lie in q.box)
    }
    sources_tally(s, emitted, removed);
    if (emitted || removed) s->stats.paths |= FLUID_PATH_SOURCES;
    return FLUID_OK;
}

// ---- the bodies of the set / stats entry points of both kinds of handle (the wrappers guard the kind) -------------------------
int fl::source_set(fluid_sim* s, int32_t slot, const fluid_source_t* src)
{
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
    if (!index_box(s, src->lo, src->hi, b)) return fail(FLUID_ERR_ARG, "source box empty or off the grid");
    if (src->per_cell < 1 || src->per_cell > 64) return fail(FLUID_ERR_ARG, "per_cell must be in 1..64");
    if (src->mode != FLUID_SOURCE_ADD && src->mode != FLUID_SOURCE_FILL) return fail(FLUID_ERR_ARG, "bad source mode");
    if (src->vel_mode != FLUID_SOURCE_VEL_FIXED && src->vel_mode != FLUID_SOURCE_VEL_GRID) return fail(FLUID_ERR_ARG, "bad source vel_mode");
    if (src->every < 1) return fail(FLUID_ERR_ARG, "every must be >= 1");
    if ((double)b.cells() * src->per_cell > (double)INT32_MAX) return fail(FLUID_ERR_ARG, "source box x per_cell exceeds INT32_MAX points");
    int rc = ensure_sums(s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s->st));
    if (q.buf) hipFree(q.buf);
    q = fluid_sim::SrcSlot{};
    HIPCHK(hipMalloc((void**)&q.buf, slot_bytes(s, b)));
    q.src = *src;
    q.box = b;
    q.on = true;
    return FLUID_OK;
}

int fl::sink_set(fluid_sim* s, int32_t slot, const int32_t lo[3], const int32_t hi[3])
{
    if (slot < 0 || slot >= FLUID_MAX_SINKS) return fail(FLUID_ERR_ARG, "sink slot out of range");
    if (!lo) {
        s->sink_on[slot] = false;
        return FLUID_OK;
    }
    Box b;
    if (!hi || !index_box(s, lo, hi, b)) return fail(FLUID_ERR_ARG, "sink box empty or off the grid");
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = ensure_sums(s);
    if (rc) return rc;
    s->sink[slot] = b;
    s->sink_on[slot] = true;
    return FLUID_OK;
}

int fl::source_stats(const fluid_sim* s, int64_t* emitted_last, int64_t* removed_last, int64_t* emitted_total, int64_t* removed_total)
{
    if (emitted_last) *emitted_last = s->src_emit_last;
    if (removed_last) *removed_last = s->src_rm_last;
    if (emitted_total) *emitted_total = s->src_emit_total;
    if (removed_total) *removed_total = s->src_rm_total;
    return FLUID_OK;
}

extern "C" {

int fluid_add_particles(fluid_sim_t* s, int64_t n, const double* pos, const double* vel)
{
    if (int rc = snap_guard(s, SRC_SINGLE)) return rc;
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
    if (int rc = snap_guard(s, SRC_SINGLE)) return rc;
    return source_set(s, slot, src);
}

int fluid_set_sink(fluid_sim_t* s, int32_t slot, const int32_t lo[3], const int32_t hi[3])
{
    if (int rc = snap_guard(s, SRC_SINGLE)) return rc;
    return sink_set(s, slot, lo, hi);
}

int fluid_get_source_stats(fluid_sim_t* s, int64_t* emitted_last, int64_t* removed_last, int64_t* emitted_total, int64_t* removed_total)
{
    if (int rc = snap_guard(s, SRC_SINGLE)) return rc;
    return source_stats(s, emitted_last, removed_last, emitted_total, removed_total);
}

}  // extern "C"
