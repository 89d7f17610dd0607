// Leaf snapshots of the output grid (include/fluid_hip.h, "output as non-zero leaves"): the step's density grid leaves the
// device as the list of its 8^3 leaves that hold anything but +0, instead of N^3 floats.  Kernels in kernels_output.hip.
//
// fluid_output_snapshot: k_out_mark -> launch_exclusive_scan -> (count read back: 4 bytes) -> k_out_pack on the handle's
// stream, so that the container is read before the next step's P2G clears it; the records then travel to pinned host
// memory on a second stream behind an event, while the handle's stream is free for the next fluid_step.  Two slots, each
// with its own device staging and pinned buffer ([n x 2048 B of values | n x 12 B of origins], one copy): a slot is
// written by snapshot q, q + 2, ..., so what fluid_output_wait handed out stays valid until the second following snapshot.
//
// fluid_dist_output_snapshot is the same sequence over the OWNED BLOCK of a handle's window (k_out_mark_win / k_out_pack_win):
// the global leaves that meet [own_lo, own_hi), with every voxel this rank does not own left +0, so that the ranks' lists
// merge by OR (fluid_leaf_grids_merge).  Rank-local: no transport call.  The state (slots, streams, counters) is one per handle
// and shared by both forms; when the cut planes move it is handed to the new window's handle (output_move) and the scratch
// that follows the leaf range is sized again at the next snapshot.
#include "sim.h"

using namespace fl;
#define fail fluid_fail

constexpr size_t OUT_REC = 2048 + 12;   // bytes per listed leaf: 512 floats + origin
struct OutSlot {
    char* dev = nullptr;       // device staging
    char* host = nullptr;      // pinned
    size_t cap = 0;            // leaves either buffer holds
    int n_leaves = 0;
    hipEvent_t done = nullptr;   // recorded on the copy stream behind the slot's copy
};
struct OutState {
    int off = 0, nl = 0;       // array index of the first leaf's first voxel (<= 0), leaves per axis
    long nleaf = 0;
    long scratch_cap = 0;      // leaves flags / slot / sums have room for
    int *flags = nullptr, *slot = nullptr, *sums = nullptr, *d_count = nullptr, *h_count = nullptr;
    hipStream_t copy = nullptr;
    hipEvent_t packed = nullptr;
    OutSlot s[2];
    long n_snap = 0, n_wait = 0;   // snapshots taken / waited for: snapshot q lives in slot q & 1
    long last_leaves = 0, last_bytes = 0;
};

#define OUT_GUARD(s)                                                     \
    if (!(s)) return fail(FLUID_ERR_ARG, "null handle");                 \
    if ((s)->dist) return fail(FLUID_ERR_STATE, "leaf snapshots of the output grid are single-GPU only: a decomposed handle holds a window, not the grid")

static int out_init(fluid_sim* s)
{
    if (s->out) return FLUID_OK;
    OutState* o = new OutState();
    s->out = o;   // from here on output_free releases whatever the lines below got
    const int lo = s->g.lo, hi = s->g.hi, L0 = lo & ~7;
    o->off = L0 - lo;
    o->nl = ((hi & ~7) - L0) / 8 + 1;
    o->nleaf = (long)o->nl * o->nl * o->nl;
    HIPCHK(hipMalloc((void**)&o->d_count, sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&o->h_count, sizeof(int)));
    HIPCHK(hipStreamCreateWithFlags(&o->copy, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&o->packed, hipEventDisableTiming));
    for (auto& q : o->s) HIPCHK(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
    return FLUID_OK;
}

// flags, slots and block sums for nleaf leaves (the handle's stream is idle or ordered before: hipFree waits for the device)
static int out_scratch(OutState* o, long nleaf)
{
    if (nleaf <= o->scratch_cap) return FLUID_OK;
    for (int** p : {&o->flags, &o->slot, &o->sums}) {
        if (*p) hipFree(*p);
        *p = nullptr;
    }
    o->scratch_cap = 0;
    HIPCHK(hipMalloc((void**)&o->flags, nleaf * sizeof(int)));
    HIPCHK(hipMalloc((void**)&o->slot, nleaf * sizeof(int)));
    HIPCHK(hipMalloc((void**)&o->sums, (nleaf / 2048 + 16) * sizeof(int)));
    o->scratch_cap = nleaf;
    return FLUID_OK;
}

// the owned block of the handle's window and the global leaves that meet it
static int out_window(fluid_sim* s, OutWin& w)
{
    int32_t org[3], dims[3], olo[3], ohi[3];
    int rc = fluid_window(s, org, dims, olo, ohi);
    if (rc) return rc;
    const int lo = s->g.lo;
    w.ny = dims[1], w.nz = dims[2];
    w.ox = org[0], w.oy = org[1], w.oz = org[2];
    w.lo = lo;
    w.off = (lo & ~7) - lo;
    for (int a = 0; a < 3; ++a) {
        if (olo[a] < org[a] || ohi[a] > org[a] + dims[a] || ohi[a] <= olo[a] || olo[a] < 0 || ohi[a] > s->g.N)
            return fail(FLUID_ERR_STATE, "the owned block does not lie inside the window");
        w.olo[a] = olo[a], w.ohi[a] = ohi[a];
        w.l0[a] = (olo[a] - w.off) >> 3;
        w.nl[a] = ((ohi[a] - 1 - w.off) >> 3) - w.l0[a] + 1;
    }
    if (w.nl[2] > 136) return fail(FLUID_ERR_ARG, "leaf snapshots need at most 136 leaves along z");
    return FLUID_OK;
}

void fl::output_free(fluid_sim* s)
{
    OutState* o = s->out;
    if (!o) return;
    if (o->copy) hipStreamSynchronize(o->copy);
    for (auto& q : o->s) {
        if (q.dev) hipFree(q.dev);
        if (q.host) hipHostFree(q.host);
        if (q.done) hipEventDestroy(q.done);
    }
    for (void* p : {(void*)o->flags, (void*)o->slot, (void*)o->sums, (void*)o->d_count})
        if (p) hipFree(p);
    if (o->h_count) hipHostFree(o->h_count);
    if (o->packed) hipEventDestroy(o->packed);
    if (o->copy) hipStreamDestroy(o->copy);
    delete o;
    s->out = nullptr;
}

// room for n leaves in the slot (its earlier contents were handed out two snapshots ago: no longer promised)
static int out_grow(OutSlot& q, size_t n)
{
    if (n <= q.cap) return FLUID_OK;
    if (q.dev) hipFree(q.dev);
    if (q.host) hipHostFree(q.host);
    q.dev = q.host = nullptr;
    q.cap = 0;
    const size_t cap = n + n / 2 + 64;
    HIPCHK(hipMalloc((void**)&q.dev, cap * OUT_REC));
    HIPCHK(hipHostMalloc((void**)&q.host, cap * OUT_REC));
    q.cap = cap;
    return FLUID_OK;
}

// mark -> scan -> count -> pack -> copy; w == nullptr: the whole grid of a one-GPU handle (k_out_mark / k_out_pack)
static int out_capture(fluid_sim* s, const OutWin* w)
{
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = out_init(s);
    if (rc) return rc;
    OutState* o = s->out;
    if (o->n_snap - o->n_wait >= 2) return fail(FLUID_ERR_STATE, "two output snapshots are waiting for fluid_output_wait");
    const long nleaf = w ? w->leaves() : o->nleaf;
    if ((rc = out_scratch(o, nleaf))) return rc;
    OutSlot& q = o->s[o->n_snap & 1];
    const int N = s->g.N;
    if (w) launch_out_mark_win(s->st, s->container, *w, o->flags);
    else launch_out_mark(s->st, s->container, N, o->off, o->nl, o->flags);
    launch_exclusive_scan(s->st, o->flags, o->slot, nleaf, o->sums, o->d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(o->h_count, o->d_count, sizeof(int), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    const int n = *o->h_count;
    if (n < 0 || (long)n > nleaf) return fail(FLUID_ERR_HIP, "leaf count out of range");
    if ((rc = out_grow(q, (size_t)n))) return rc;
    q.n_leaves = n;
    if (n > 0) {
        float* values = (float*)q.dev;
        int* origin = (int*)(q.dev + (size_t)n * 2048);
        if (w) launch_out_pack_win(s->st, s->container, *w, o->flags, o->slot, values, origin);
        else launch_out_pack(s->st, s->container, N, s->g.lo, o->off, o->nl, o->flags, o->slot, values, origin);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(o->packed, s->st));
        HIPCHK(hipStreamWaitEvent(o->copy, o->packed, 0));
        HIPCHK(hipMemcpyAsync(q.host, q.dev, (size_t)n * OUT_REC, hipMemcpyDeviceToHost, o->copy));
    }
    HIPCHK(hipEventRecord(q.done, o->copy));
    o->n_snap++;
    o->last_leaves = n;
    o->last_bytes = (long)((size_t)n * OUT_REC) + FLUID_OUTPUT_HEADER_BYTES;
    return FLUID_OK;
}

static int out_wait(fluid_sim* s, fluid_leaf_grid_t* out)
{
    if (!out) return fail(FLUID_ERR_ARG, "null argument");
    OutState* o = s->out;
    if (!o || o->n_wait >= o->n_snap) return fail(FLUID_ERR_STATE, "no output snapshot is outstanding");
    OutSlot& q = o->s[o->n_wait & 1];
    HIPCHK(hipEventSynchronize(q.done));
    out->n = s->g.N;
    out->n_leaves = q.n_leaves;
    out->values = q.n_leaves ? (const float*)q.host : nullptr;
    out->origin = q.n_leaves ? (const int32_t*)(q.host + (size_t)q.n_leaves * 2048) : nullptr;
    o->n_wait++;
    return FLUID_OK;
}

static bool out_due(const fluid_sim* s) { return s->out_every > 0 && s->n_steps % s->out_every == 0; }

int fl::output_auto_check(fluid_sim* s)
{
    if (out_due(s) && s->out && s->out->n_snap - s->out->n_wait >= 2)
        return fail(FLUID_ERR_STATE, "fluid_step: this step takes an output snapshot (fluid_dist_output_every) and two are waiting for fluid_dist_output_wait");
    return FLUID_OK;
}

int fl::output_auto(fluid_sim* s)
{
    if (!out_due(s)) return FLUID_OK;
    OutWin w;
    int rc = out_window(s, w);
    return rc ? rc : out_capture(s, &w);
}

void fl::output_move(fluid_sim* from, fluid_sim* to)
{
    output_free(to);
    to->out = from->out;
    from->out = nullptr;
    to->out_every = from->out_every;
    to->n_steps = from->n_steps;
}

extern "C" {

int fluid_output_snapshot(fluid_sim_t* s)
{
    OUT_GUARD(s);
    return out_capture(s, nullptr);
}

int fluid_output_wait(fluid_sim_t* s, fluid_leaf_grid_t* out)
{
    OUT_GUARD(s);
    return out_wait(s, out);
}

int fluid_output_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host)
{
    OUT_GUARD(s);
    const int lo = s->g.lo, hi = s->g.hi;
    const int64_t nl = ((hi & ~7) - (lo & ~7)) / 8 + 1;
    if (leaves_in_grid) *leaves_in_grid = nl * nl * nl;
    if (leaves_listed) *leaves_listed = s->out ? s->out->last_leaves : 0;
    if (bytes_to_host) *bytes_to_host = s->out ? s->out->last_bytes : 0;
    return FLUID_OK;
}

int fluid_dist_output_snapshot(fluid_sim_t* s)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    OutWin w;
    int rc = out_window(s, w);
    return rc ? rc : out_capture(s, &w);
}

int fluid_dist_output_wait(fluid_sim_t* s, fluid_leaf_grid_t* out)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    return out_wait(s, out);
}

int fluid_dist_output_stats(fluid_sim_t* s, int64_t* leaves_in_block, int64_t* leaves_listed, int64_t* bytes_to_host)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    OutWin w;
    int rc = out_window(s, w);
    if (rc) return rc;
    if (leaves_in_block) *leaves_in_block = w.leaves();
    if (leaves_listed) *leaves_listed = s->out ? s->out->last_leaves : 0;
    if (bytes_to_host) *bytes_to_host = s->out ? s->out->last_bytes : 0;
    return FLUID_OK;
}

int fluid_dist_output_every(fluid_sim_t* s, int32_t every)
{
    if (!s || every < 0) return fail(FLUID_ERR_ARG, "null handle, or every < 0");
    s->out_every = every;
    return FLUID_OK;
}

}  // extern "C"
