// Leaf snapshots of the output grid (include/fluid_hip.h, "output as non-zero leaves"): the step's density grid leaves the
// device as the list of its 8^3 leaves that hold anything but +0, instead of N^3 floats.  Kernels in kernels_output.hip.
//
// A snapshot works on the OWNED BLOCK of the handle's window (OutWin): k_out_mark -> launch_exclusive_scan -> (count read back:
// 4 bytes) -> k_out_pack on the handle's stream, so that the container is read before the next step's P2G clears it; the records
// ([n x 2048 B of values | n x 12 B of origins]) then leave through the handle's ring of two slots (snap_ring.h).
//
// fluid_output_snapshot: one GPU, where window = grid = owned block.  fluid_dist_output_snapshot: a rank of a decomposed run: the
// global leaves that meet [own_lo, own_hi), with every voxel this rank does not own left +0, so that the ranks' lists merge by OR
// (fluid_leaf_grids_merge).  Rank-local: no transport call.  The state (ring, counters, scratch) is one per handle and shared by
// both forms; when the cut planes move it is handed to the new window's handle (output_move) and the scratch that follows the leaf
// range is sized again at the next snapshot.
#include "sim.h"

using namespace fl;
#define fail fluid_fail

constexpr size_t OUT_REC = 2048 + 12;   // bytes per listed leaf: 512 floats + origin
struct OutState {
    long scratch_cap = 0;      // leaves flags / slot / sums have room for
    int *flags = nullptr, *slot = nullptr, *sums = nullptr, *d_count = nullptr, *h_count = nullptr;
    SnapRing ring;
    int n_leaves[2] = {0, 0};  // per slot of the ring
    long last_leaves = 0, last_bytes = 0;
};

static const char* const OUT_SINGLE = "leaf snapshots of the output grid are single-GPU only: a decomposed handle holds a window, not the grid";

static int out_init(fluid_sim* s)
{
    if (s->out) return FLUID_OK;
    OutState* o = new OutState();
    s->out = o;   // from here on output_free releases whatever the lines below got
    HIPCHK(hipMalloc((void**)&o->d_count, sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&o->h_count, sizeof(int)));
    return snap_init(o->ring);
}

// flags, slots and block sums for nleaf leaves (the handle's stream is idle or ordered before: hipFree waits for the device)
static int out_scratch(OutState* o, long nleaf)
{
    if (nleaf <= o->scratch_cap) return FLUID_OK;
    o->scratch_cap = 0;
    HIPCHK(regrow(o->flags, (size_t)nleaf));
    HIPCHK(regrow(o->slot, (size_t)nleaf));
    HIPCHK(regrow(o->sums, (size_t)nleaf / 2048 + 16));
    o->scratch_cap = nleaf;
    return FLUID_OK;
}

// the owned block of the handle's window and the global leaves that meet it; a one-GPU handle owns its whole grid (fluid_window)
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
    snap_free(o->ring);
    for (void* p : {(void*)o->flags, (void*)o->slot, (void*)o->sums, (void*)o->d_count})
        if (p) hipFree(p);
    if (o->h_count) hipHostFree(o->h_count);
    delete o;
    s->out = nullptr;
}

// mark -> scan -> count -> pack -> copy
static int out_capture(fluid_sim* s, const OutWin& w)
{
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = out_init(s);
    if (rc) return rc;
    OutState* o = s->out;
    if (snap_full(o->ring)) return fail(FLUID_ERR_STATE, "two output snapshots are waiting for fluid_output_wait");
    const long nleaf = w.leaves();
    if ((rc = out_scratch(o, nleaf))) return rc;
    const int k = snap_slot(o->ring);
    SnapSlot& q = o->ring.s[k];
    launch_out_mark(s->st, s->container, w, o->flags);
    launch_exclusive_scan(s->st, o->flags, o->slot, nleaf, o->sums, o->d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(o->h_count, o->d_count, sizeof(int), hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    const int n = *o->h_count;
    if (n < 0 || (long)n > nleaf) return fail(FLUID_ERR_HIP, "leaf count out of range");
    if ((rc = snap_reserve(q, (size_t)n * OUT_REC, 64 * OUT_REC))) return rc;
    o->n_leaves[k] = n;
    if (n > 0) {
        launch_out_pack(s->st, s->container, w, o->flags, o->slot, (float*)q.dev, (int*)(q.dev + (size_t)n * 2048));
        HIPCHK(hipGetLastError());
    }
    if ((rc = snap_commit(o->ring, s->st, (size_t)n * OUT_REC))) return rc;
    o->last_leaves = n;
    o->last_bytes = (long)((size_t)n * OUT_REC) + FLUID_OUTPUT_HEADER_BYTES;
    return FLUID_OK;
}

static int out_wait(fluid_sim* s, fluid_leaf_grid_t* out)
{
    if (!out) return fail(FLUID_ERR_ARG, "null argument");
    OutState* o = s->out;
    int k = -1, rc = o ? snap_next_wait(o->ring, &k) : FLUID_OK;
    if (rc) return rc;
    if (k < 0) return fail(FLUID_ERR_STATE, "no output snapshot is outstanding");
    const char* host = o->ring.s[k].host;
    const int n = o->n_leaves[k];
    out->n = s->g.N;
    out->n_leaves = n;
    out->values = n ? (const float*)host : nullptr;
    out->origin = n ? (const int32_t*)(host + (size_t)n * 2048) : nullptr;
    return FLUID_OK;
}

static int out_snapshot(fluid_sim* s)
{
    OutWin w;
    int rc = out_window(s, w);
    return rc ? rc : out_capture(s, w);
}

static bool out_due(const fluid_sim* s) { return s->out_every > 0 && s->n_steps % s->out_every == 0; }

int fl::output_auto_check(fluid_sim* s)
{
    if (out_due(s) && s->out && snap_full(s->out->ring))
        return fail(FLUID_ERR_STATE, "fluid_step: this step takes an output snapshot (fluid_dist_output_every) and two are waiting for fluid_dist_output_wait");
    return FLUID_OK;
}

int fl::output_auto(fluid_sim* s)
{
    return out_due(s) ? out_snapshot(s) : FLUID_OK;
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
    int rc = snap_guard(s, OUT_SINGLE);
    return rc ? rc : out_snapshot(s);
}

int fluid_output_wait(fluid_sim_t* s, fluid_leaf_grid_t* out)
{
    int rc = snap_guard(s, OUT_SINGLE);
    return rc ? rc : out_wait(s, out);
}

int fluid_output_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host)
{
    if (int rc = snap_guard(s, OUT_SINGLE)) return rc;
    const int64_t nl = grid_leaves(s->g);
    if (leaves_in_grid) *leaves_in_grid = nl * nl * nl;
    if (leaves_listed) *leaves_listed = s->out ? s->out->last_leaves : 0;
    if (bytes_to_host) *bytes_to_host = s->out ? s->out->last_bytes : 0;
    return FLUID_OK;
}

int fluid_dist_output_snapshot(fluid_sim_t* s)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    return out_snapshot(s);
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
