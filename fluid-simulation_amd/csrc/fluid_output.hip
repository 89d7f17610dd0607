// Leaf snapshots of the output grid (include/fluid_hip.h, "output as non-zero leaves"): the step's density grid leaves the
// device as the list of its 8^3 leaves that hold anything but +0, instead of N^3 floats.  Kernels in kernels_output.hip.
//
// fluid_output_snapshot: k_out_mark -> launch_exclusive_scan -> (count read back: 4 bytes) -> k_out_pack on the handle's
// stream, so that the container is read before the next step's P2G clears it; the records then travel to pinned host
// memory on a second stream behind an event, while the handle's stream is free for the next fluid_step.  Two slots, each
// with its own device staging and pinned buffer ([n x 2048 B of values | n x 12 B of origins], one copy): a slot is
// written by snapshot q, q + 2, ..., so what fluid_output_wait handed out stays valid until the second following snapshot.
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
    HIPCHK(hipMalloc((void**)&o->flags, o->nleaf * sizeof(int)));
    HIPCHK(hipMalloc((void**)&o->slot, o->nleaf * sizeof(int)));
    HIPCHK(hipMalloc((void**)&o->sums, (o->nleaf / 2048 + 16) * sizeof(int)));
    HIPCHK(hipMalloc((void**)&o->d_count, sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&o->h_count, sizeof(int)));
    HIPCHK(hipStreamCreateWithFlags(&o->copy, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&o->packed, hipEventDisableTiming));
    for (auto& q : o->s) HIPCHK(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
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

extern "C" {

int fluid_output_snapshot(fluid_sim_t* s)
{
    OUT_GUARD(s);
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = out_init(s);
    if (rc) return rc;
    OutState* o = s->out;
    if (o->n_snap - o->n_wait >= 2) return fail(FLUID_ERR_STATE, "two output snapshots are waiting for fluid_output_wait");
    OutSlot& q = o->s[o->n_snap & 1];
    const int N = s->g.N;
    launch_out_mark(s->st, s->container, N, o->off, o->nl, o->flags);
    launch_exclusive_scan(s->st, o->flags, o->slot, o->nleaf, o->sums, o->d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(o->h_count, o->d_count, sizeof(int), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    const int n = *o->h_count;
    if (n < 0 || (long)n > o->nleaf) return fail(FLUID_ERR_HIP, "leaf count out of range");
    if ((rc = out_grow(q, (size_t)n))) return rc;
    q.n_leaves = n;
    if (n > 0) {
        launch_out_pack(s->st, s->container, N, s->g.lo, o->off, o->nl, o->flags, o->slot, (float*)q.dev, (int*)(q.dev + (size_t)n * 2048));
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

int fluid_output_wait(fluid_sim_t* s, fluid_leaf_grid_t* out)
{
    OUT_GUARD(s);
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

}  // extern "C"
