// Level-set snapshots of the particles (include/fluid_hip.h, "liquid surface"): the narrow-band signed distance to the spheres
// around the particles leaves the device as the list of OpenVDB's 8^3 leaves that hold anything but inactive +bg.  Kernels in
// kernels_sdf.hip.
//
// fluid_sdf_snapshot, all on the handle's stream: bounding box of the counted particles' base cells (24 bytes read back: it sizes
// everything that follows) -> count per cell of the box, exclusive scan, scatter of the positions into cell order -> search over
// the leaves of the box dilated by 4 cells (values, masks and a listed flag per leaf of that range) -> exclusive scan of the
// flags (count read back: 4 bytes) -> pack into the slot's device staging ([n x 2048 B of values | n x 64 B of masks | n x 12 B
// of origins]); the records then leave through the level set's own ring of two slots (snap_ring.h).
// The particle arrays are only read; key, slot, cell_count, cell_start, the second particle buffer and every field stay as they
// are, and `binned` keeps holding: the next step's sort starts from what FLIPadvect left, as if no snapshot had been taken.
//
// fluid_dist_sdf_snapshot is the same sequence on a decomposed handle ("liquid surface (decomposed runs)"): the rank's LIVE
// particles (k_sdf_bbox<true> / k_sdf_count<true> pass over the entries marked PID_DEAD), global coordinates, every leaf they reach
// whether the rank owns it or not.  Rank-local: no transport call; the ranks' lists merge on the host (fluid_sdf_grids_merge,
// vdb_sdf_writer.cpp).  The state is one per handle and shared by both forms; when the cut planes move it is handed to the new
// window's handle (sdf_move), so lists handed out or in flight stay valid.
//
// The front half (sdf_begin, sdf_front: everything up to and including the search) is also the front half of fluid_mesh_snapshot
// (fluid_mesh.hip), which works on the search's scratch in place of the pack.
//
// fluid_sdf_snapshot_filtered / fluid_mesh_snapshot_filtered ("liquid surface, smoothed"; kernels_sdf_filter.hip): the front half
// ends with the filter's box passes, one launch each, 3 per iteration (x, z, y), from tv to tv2 and back; what follows reads
// whichever buffer the last pass wrote.  tv2 exists from the handle's first filtered snapshot on.  The order of passes, offset
// steps and tracks of all three forms, and the limits of their arguments, are sdf_filter_plan.h's, shared with the host functions
// (sdf_filter_host.cpp); sdf_front supplies what each of them launches.
//
// fluid_sdf_set_track ("liquid surface, renormalised"; kernels_sdf_track.hip): with the setting on, every filter of the front half
// runs its tracked form: a track (N normalisation passes, one launch each, ping-pong like the box passes; the trim rides on the
// last) after every iteration's three box passes and after every step of the offset, which is then taken in steps of at most
// dx / 2 by the offset kernel.  `flags` keeps meaning "this leaf's values are valid" throughout (neighbour blocks read it); after
// the last trim one more launch derives the LIST flags (lflags) from what the trim left, and the scan and the pack run off those.
// lflags exists from the handle's first tracked snapshot on.
//
// fluid_sdf_set_track_grow ("liquid surface, grown band"; kernels_sdf_grow.hip): with the setting on, every track begins with one
// dilation launch, and the range is the particles' box dilated by f->dilate + T cells, T = the number of tracks the filter runs,
// which the host knows before anything is sized.  The launch reads flags / tm and writes flags2 / tm2 (ping-pong: neighbour blocks
// of the launch read this leaf's flag and words); the host swaps the two pairs after it, and whoever follows — passes, relist,
// pack, mesh, ray caster — is handed the pair that is current (f->flags, f->tm).  The search of the next snapshot writes flags / tm
// again, every leaf of its range, so nothing of an earlier snapshot is read.  flags2 and tm2 exist from the handle's first grown
// snapshot on.
//
// fluid_sdf_set_filter_kind ("liquid surface, flows"; kernels_sdf_flow.hip): with a kind other than BOX every filter of the front
// half runs that kind's one pass per iteration in place of the three box passes: one launch, ping-pong between the same two value
// buffers; tracks, growing and the offset follow it exactly as they follow a box iteration.
//
// fluid_sdf_set_surface ("liquid surface, averaged positions"; kernels_sdf_avg.hip): with kind AVERAGED the front half launches
// k_sdf_search_avg in place of k_sdf_search, behind the same bin, scan and scatter; tv / tm / flags mean what they meant, so filters,
// tracks, growth, pack, mesh and ray caster follow unchanged.  Attribute snapshots and the rank records of decomposed runs are
// refused under it (FLUID_ERR_STATE).
//
// fluid_dist_sdf_snapshot_avg ("liquid surface, averaged positions (decomposed runs)"): the rank record of the averaged surface is a
// fourth kind of snapshot in the same ring.  The surface comes with the call, not from the handle's setting; the front half launches
// k_sdf_search_avg<true>, which writes dist2 into tmin and the four sums into tsum (32 B per voxel of the range, allocated by the
// handle's first such snapshot) and flags the leaves with m < max(max2, h2); k_sdf_pack_avg lists them:
// [n x 2048 B of dist2 | n x 16384 B of sums | n x 12 B of origins].  No values, no masks: the merge on the host
// (fluid_sdf_avg_grids_merge, sdf_avg_host.cpp) makes them.  Only fluid_dist_sdf_wait_avg takes such a snapshot, and it takes no other.
//
// fluid_sdf_set_trails ("liquid surface, velocity trails"; kernels_sdf_trail.hip): with the setting on the front half first expands
// the live particles into instances (count pass with the instances' base-cell box and their total, 24 + 8 bytes read back; scan;
// write pass), then bins the INSTANCES behind the same count and scan, with a scatter that carries the radius, and launches
// k_sdf_search_rad in place of k_sdf_search; tv / tm / flags mean what they meant.  Scratch of its own: icnt / ioff per particle, and
// per instance 60 bytes: ipos and ir (28), place and spos, which are the spheres' arrays sized for the instances (28), and sr (4);
// allocated by the handle's first snapshot under the setting.  Attribute snapshots and the spheres' rank records are refused under it.
//
// fluid_dist_sdf_snapshot_trails ("liquid surface, velocity trails (decomposed runs)"): the same front half with the trails handed in
// (spheres and these trails: no setting of the handle is read or changed) and, on a decomposed handle, the <true> forms of the two
// expansion passes, which pass over the dead entries and count the live ones (8 more bytes read back).  The instances have no pid: they
// are binned by k_sdf_count<false>.  The record is a plain one (kind 0), taken by fluid_dist_sdf_wait; the counters are its own
// (dist_trail_*), so that fluid_sdf_trails_stats keeps meaning "of the last snapshot under the setting".
//
// fluid_sdf_snapshot_attr / fluid_mesh_snapshot_attr ("liquid surface, attributes"): the scatter also writes each sorted position's
// index in the live arrays (ssrc), the search keeps the closest particle beside the minimum and writes its id and velocity per voxel
// (tid, tvel), and the pack lists them.  ssrc, tid and tvel exist from the handle's first attribute snapshot on.  An attribute
// snapshot is one more kind of snapshot in the same ring: its record is [n x 2048 B of values | n x 2048 B of ids |
// n x 6144 B of velocities | n x 64 B of masks | n x 12 B of origins] (the 16-byte copies of the pack stay aligned for every n).
// Once a slot has held an attribute snapshot it keeps room for attributes (wide); a plain snapshot uses the front of it.
//
// fluid_dist_sdf_snapshot_attr ("liquid surface, attributes (decomposed runs)"): the attribute snapshot of the rank's live particles
// whose search also writes the squared distance m per voxel (tmin) and whose record lists it: [values | ids | velocities |
// n x 2048 B of dist2 | masks | origins].  The ids come through ssrc from the pid of the handle's current arrays (global ids on a
// decomposed handle; a dead entry is never scattered, so never a winner).  tmin exists from the handle's first such snapshot on; a
// slot keeps room for the longest record per leaf it has held (wide = 0, 1, 2).
#include "sim.h"
#include "sdf_filter_plan.h"
#include "sdf_avg_def.h"
#include "sdf_trail_def.h"

using namespace fl;
#define fail fluid_fail

constexpr size_t SDF_REC = FLUID_SDF_LEAF_BYTES;
struct SdfMeta {               // per slot of the ring
    int wide = 0;              // the slot is sized for leaves of this kind (the longest it has held)
    int attr = 0;              // the snapshot in the slot: 0 plain, 1 with attributes, 2 with attributes and dist2, 3 an averaged rank record
    int n_leaves = 0;
    float bg = 0, R = 0, w = 0;
    float dxf = 0, hf = 0;     // kind 3: what the merge needs beside them
};
constexpr int SDF_AVG_RECORD = 3;
struct SdfState {
    // scratch: cells of the particles' box, particles, leaves of the dilated box
    long cell_cap = 0, part_cap = 0, leaf_cap = 0;
    int *cnt = nullptr, *start = nullptr, *cell_sums = nullptr;
    int* place = nullptr;
    double* spos = nullptr;    // sorted x | y | z, part_cap each
    float* tv = nullptr;
    float* tv2 = nullptr;      // the box passes' second buffer, leaf_cap x 512 like tv: allocated once a filtered snapshot was asked for
    bool filtered = false;
    int* lflags = nullptr;     // the list flags after a trim, leaf_cap like flags: allocated once a tracked snapshot was asked for
    bool tracked = false;
    fluid_sdf_track_t track{0, 0, FLUID_SDF_TRACK_FIRST_BIAS};   // fluid_sdf_set_track: passes per track and the trim (0 / 0: off)
    int* flags2 = nullptr;     // the dilation's second flags and masks (leaf_cap, leaf_cap x 8): allocated once a grown snapshot was asked for
    uint64_t* tm2 = nullptr;
    bool grown = false;
    bool track_grow = false;   // fluid_sdf_set_track_grow
    int kind = FLUID_SDF_FILTER_BOX;   // fluid_sdf_set_filter_kind
    fluid_sdf_surface_t surface{FLUID_SDF_SURFACE_SPHERES, 0, 0.0};   // fluid_sdf_set_surface
    // attributes: index in the live arrays per sorted position (part_cap), winner's id (leaf_cap x 512) and velocity (leaf_cap x 3 x 512)
    // per voxel: allocated once an attribute snapshot was asked for
    int* ssrc = nullptr;
    uint32_t* tid = nullptr;
    float* tvel = nullptr;
    bool attr = false;
    float* tmin = nullptr;     // m per voxel (leaf_cap x 512): allocated once a snapshot with dist2 was asked for
    bool dist2 = false;
    uint64_t* tsum = nullptr;  // SW, SX, SY, SZ per voxel ([leaf_cap][4][512]): allocated once an averaged rank record was asked for
    bool avgrec = false;
    // velocity trails (fluid_sdf_set_trails): instances per particle and their scan (tpart_cap), the instances and their radii,
    // unsorted and sorted (inst_cap): allocated once a snapshot under the setting was asked for
    fluid_sdf_trails_t trails{0.0, 0.0, 0.0, 0, 0};
    bool trails_on = false;
    long tpart_cap = 0, inst_cap = 0;
    int *icnt = nullptr, *ioff = nullptr, *isums = nullptr;
    double* ipos = nullptr;    // x | y | z, inst_cap each
    float *ir = nullptr, *sr = nullptr;
    int64_t trail_particles = 0, trail_instances = 0;   // of the last snapshot under the setting
    int64_t dist_trail_particles = 0, dist_trail_instances = 0;   // of the last fluid_dist_sdf_snapshot_trails
    uint64_t* tm = nullptr;
    int *flags = nullptr, *slot = nullptr, *leaf_sums = nullptr;
    unsigned* visits = nullptr;   // FLUID_SDF_VISITS=1 only
    bool count_visits = false;
    bool grow_stats = false;      // FLUID_SDF_GROW_STATS=1 only
    int *d_small = nullptr, *h_small = nullptr;   // box[6], cell total, listed count, the trails' 64-bit instance total and live count
    SnapRing ring;
    SdfMeta m[2];
    long last_leaves = 0, last_bytes = 0;
};

static const char* const SDF_SINGLE = "level-set snapshots are single-GPU only: a decomposed handle holds a block of the particles (fluid_dist_sdf_*)";
static const char* const SDF_FILT_SINGLE = "filtered level-set snapshots are single-GPU only: a mean of per-block minima is not the mean of the minimum; filter the merged list on the host (fluid_sdf_filter)";

static const char* const SDF_GROW_SINGLE = "grown level-set snapshots are single-GPU only: a decomposed handle's filter runs on the merged list on the host (fluid_sdf_filter_grown)";
static const char* const SDF_KIND_SINGLE = "level-set flows are single-GPU only: a decomposed handle's filter runs on the merged list on the host (fluid_sdf_flow)";
static const char* const SDF_AVG_SINGLE = "the averaged-position surface as a handle's setting is single-GPU only: a decomposed handle gives the rank record of the minimum and the four sums (fluid_dist_sdf_snapshot_avg), merged on the host (fluid_sdf_avg_grids_merge)";
static const char* const SDF_AVG_ATTR = "the averaged-position surface carries no attributes: an average of positions has no closest particle (fluid_sdf_set_surface)";
static const char* const SDF_AVG_DIST = "fluid_dist_sdf_snapshot gives the spheres' rank record: the averaged-position surface has a rank record of its own, which takes the surface as an argument (fluid_dist_sdf_snapshot_avg)";
static const char* const SDF_TRAIL_SINGLE = "velocity trails as a handle's setting are single-GPU only: a decomposed handle gives the rank record of its live particles' instances, which takes the trails as an argument (fluid_dist_sdf_snapshot_trails), merged on the host (fluid_sdf_grids_merge)";
static const char* const SDF_TRAIL_ATTR = "velocity trails carry no attributes (fluid_sdf_set_trails)";
static const char* const SDF_TRAIL_DIST = "fluid_dist_sdf_snapshot gives the spheres' rank record: it is refused while velocity trails are set (fluid_sdf_set_trails); the trails' rank record takes them as an argument (fluid_dist_sdf_snapshot_trails)";
static const char* const SDF_TRAIL_AVG = "velocity trails and the averaged-position surface exclude each other (fluid_sdf_set_trails, fluid_sdf_set_surface)";
static const char* const SDF_TRACK_SINGLE = "tracked level-set snapshots are single-GPU only: a decomposed handle's filter runs on the merged list on the host (fluid_sdf_filter_tracked)";

static int sdf_init(fluid_sim* s)
{
    if (s->sdf) return FLUID_OK;
    SdfState* o = new SdfState();
    s->sdf = o;   // from here on sdf_free releases whatever the lines below got
    if (const char* e = getenv("FLUID_SDF_VISITS")) o->count_visits = atoi(e) != 0;   // developer knob (tools/sdf_cost.py)
    if (const char* e = getenv("FLUID_SDF_GROW_STATS")) o->grow_stats = atoi(e) != 0;   // developer knob (tools/grow_cost.py)
    HIPCHK(hipMalloc((void**)&o->d_small, 12 * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&o->h_small, 12 * sizeof(int)));
    return snap_init(o->ring);
}

void fl::sdf_free(fluid_sim* s)
{
    SdfState* o = s->sdf;
    if (!o) return;
    snap_free(o->ring);
    for (void* p : {(void*)o->cnt, (void*)o->start, (void*)o->cell_sums, (void*)o->place, (void*)o->spos, (void*)o->tv, (void*)o->tv2, (void*)o->lflags, (void*)o->flags2, (void*)o->tm2, (void*)o->ssrc, (void*)o->tid, (void*)o->tvel, (void*)o->tmin, (void*)o->tsum, (void*)o->tm, (void*)o->flags,
                    (void*)o->icnt, (void*)o->ioff, (void*)o->isums, (void*)o->ipos, (void*)o->ir, (void*)o->sr, (void*)o->slot, (void*)o->leaf_sums, (void*)o->visits, (void*)o->d_small})
        if (p) hipFree(p);
    if (o->h_small) hipHostFree(o->h_small);
    delete o;
    s->sdf = nullptr;
}

// (the handle's stream is idle here: every caller has just waited for a read-back on it)
static int sdf_scratch(SdfState* o, long cells, long parts, long leaves, bool filtered, bool attr, bool dist2, bool tracked, bool grown, bool avgrec)
{
    if (avgrec && !o->avgrec) {   // the first averaged rank record of the handle: tsum beside whatever there is
        o->avgrec = true;
        if (o->leaf_cap > 0) HIPCHK(regrow(o->tsum, (size_t)o->leaf_cap * 2048));
    }
    if (grown && !o->grown) {   // the first grown snapshot of the handle: flags2 and tm2 beside whatever flags and tm there are
        o->grown = true;
        if (o->leaf_cap > 0) {
            HIPCHK(regrow(o->flags2, (size_t)o->leaf_cap));
            HIPCHK(regrow(o->tm2, (size_t)o->leaf_cap * 8));
        }
    }
    if (tracked && !o->tracked) {   // the first tracked snapshot of the handle: lflags beside whatever flags there are
        o->tracked = true;
        if (o->leaf_cap > 0) HIPCHK(regrow(o->lflags, (size_t)o->leaf_cap));
    }
    if (dist2 && !o->dist2) {   // the first snapshot with dist2 of the handle: tmin beside whatever there is
        o->dist2 = true;
        if (o->leaf_cap > 0) HIPCHK(regrow(o->tmin, (size_t)o->leaf_cap * 512));
    }
    if (attr && !o->attr) {   // the first attribute snapshot of the handle: ssrc, tid and tvel beside whatever there is
        o->attr = true;
        if (o->part_cap > 0) HIPCHK(regrow(o->ssrc, (size_t)o->part_cap));
        if (o->leaf_cap > 0) {
            HIPCHK(regrow(o->tid, (size_t)o->leaf_cap * 512));
            HIPCHK(regrow(o->tvel, (size_t)o->leaf_cap * 1536));
        }
    }
    if (filtered && !o->filtered) {   // the first filtered snapshot of the handle: tv2 beside whatever tv there is
        o->filtered = true;
        if (o->leaf_cap > 0) HIPCHK(regrow(o->tv2, (size_t)o->leaf_cap * 512));
    }
    if (cells > o->cell_cap) {
        o->cell_cap = 0;
        const long cap = cells + cells / 4 + 64;
        HIPCHK(regrow(o->cnt, (size_t)cap + 8));
        HIPCHK(regrow(o->start, (size_t)cap + 8));
        HIPCHK(regrow(o->cell_sums, (size_t)cap / 2048 + 16));
        o->cell_cap = cap;
    }
    if (parts > o->part_cap) {
        o->part_cap = 0;
        const long cap = parts + parts / 8 + 64;
        HIPCHK(regrow(o->place, (size_t)cap));
        HIPCHK(regrow(o->spos, (size_t)3 * cap));
        if (o->attr) HIPCHK(regrow(o->ssrc, (size_t)cap));
        o->part_cap = cap;
    }
    if (leaves > o->leaf_cap) {
        o->leaf_cap = 0;
        const long cap = leaves + leaves / 4 + 64;
        HIPCHK(regrow(o->tv, (size_t)cap * 512));
        if (o->filtered) HIPCHK(regrow(o->tv2, (size_t)cap * 512));
        if (o->attr) {
            HIPCHK(regrow(o->tid, (size_t)cap * 512));
            HIPCHK(regrow(o->tvel, (size_t)cap * 1536));
        }
        if (o->dist2) HIPCHK(regrow(o->tmin, (size_t)cap * 512));
        if (o->avgrec) HIPCHK(regrow(o->tsum, (size_t)cap * 2048));
        HIPCHK(regrow(o->tm, (size_t)cap * 8));
        HIPCHK(regrow(o->flags, (size_t)cap));
        if (o->tracked) HIPCHK(regrow(o->lflags, (size_t)cap));
        if (o->grown) {
            HIPCHK(regrow(o->flags2, (size_t)cap));
            HIPCHK(regrow(o->tm2, (size_t)cap * 8));
        }
        HIPCHK(regrow(o->slot, (size_t)cap));
        HIPCHK(regrow(o->leaf_sums, (size_t)cap / 2048 + 16));
        if (o->count_visits) HIPCHK(regrow(o->visits, (size_t)cap));
        o->leaf_cap = cap;
    }
    return FLUID_OK;
}

// The trails' scratch: per particle before the count pass, per instance once the total is known (the stream is idle at both places)
static int trail_scratch(SdfState* o, long parts, long inst)
{
    if (parts > o->tpart_cap) {
        o->tpart_cap = 0;
        const long cap = parts + parts / 8 + 64;
        HIPCHK(regrow(o->icnt, (size_t)cap));
        HIPCHK(regrow(o->ioff, (size_t)cap));
        HIPCHK(regrow(o->isums, (size_t)cap / 2048 + 16));
        o->tpart_cap = cap;
    }
    if (inst > o->inst_cap) {
        o->inst_cap = 0;
        const long cap = inst + inst / 8 + 64;
        HIPCHK(regrow(o->ipos, (size_t)3 * cap));
        HIPCHK(regrow(o->ir, (size_t)cap));
        HIPCHK(regrow(o->sr, (size_t)cap));
        o->inst_cap = cap;
    }
    return FLUID_OK;
}

// FLUID_SDF_GROW_STATS=1: how many leaves of the range are flagged (two host waits: a figure for tools/grow_cost.py, never a default)
static long sdf_count_flags(fluid_sim* s, const int* flags, long leaves)
{
    std::vector<int> h((size_t)leaves);
    if (hipMemcpyAsync(h.data(), flags, (size_t)leaves * sizeof(int), hipMemcpyDeviceToHost, s->st) != hipSuccess || hipStreamSynchronize(s->st) != hipSuccess) return -1;
    long k = 0;
    for (int v : h) k += v != 0;
    return k;
}

// The front half of a snapshot, shared with the mesh (fluid_mesh.hip).  sdf_begin: the parameters' limits, the state, the constants
// of the level set.  sdf_front: bbox (24 bytes read back: the handle's stream is waited for) -> count, scan, scatter -> search, all
// on the handle's stream; a decomposed handle (s->dist) bins its live entries only.  f->any = some particle counts; then f->g holds
// the box and the range, and tv / flags are the search's: 512 values and a listed flag per leaf of the range (the values of a leaf
// whose flag is 0 may be stale: kernels_sdf.hip).  The scratch is one per handle: whoever calls next overwrites it, in stream order.
int fl::sdf_begin(fluid_sim* s, const fluid_sdf_params_t* p, SdfFront* f, const fluid_sdf_filter_t* filt, const fluid_sdf_surface_t* sf_arg,
                  const fluid_sdf_trails_t* tr_arg)
{
    if (!p) return fail(FLUID_ERR_ARG, "null argument");
    if (filt && !plan::filter_ok(filt))
        return fail(FLUID_ERR_ARG, "level-set filter: width in 1..4, iterations in 0..16 and a finite offset are required");
    const float R = (float)p->radius, w = (float)p->half_width;
    const float mx = R + w;
    if (!(p->radius > 0) || !(R > 0.0f) || !(w >= 1.0f) || !(mx <= 4.0f))
        return fail(FLUID_ERR_ARG, "level set: radius > 0, half_width >= 1 and radius + half_width <= 4 (voxels) are required");
    HIPCHK(hipSetDevice(s->prm.device));
    int rc = sdf_init(s);
    if (rc) return rc;
    SdfGeom& g = f->g;
    g = SdfGeom{};
    g.lo = s->g.lo, g.hi = s->g.hi, g.L0 = g.lo & ~7;
    g.R = R, g.w = w, g.dxf = (float)s->prm.dx;
    g.bg = g.dxf * w;
    g.max2 = mx * mx;
    const float mn = std::fmax(0.0f, R - w);
    g.min2 = mn * mn;
    f->any = false;
    f->tv = nullptr, f->flags = nullptr, f->list = nullptr;
    const fluid_sdf_track_t* t = filt ? &s->sdf->track : nullptr;   // the argument rules: sdf_filter_plan.h
    f->track_n = t ? t->normalize : 0, f->track_trim = t && t->trim != 0;
    f->track_scheme = t ? t->scheme : FLUID_SDF_TRACK_FIRST_BIAS;
    f->grow = filt && s->sdf->track_grow;
    f->kind = filt ? s->sdf->kind : FLUID_SDF_FILTER_BOX;
    if (filt && !plan::width_ok(f->kind, filt->width))
        return fail(FLUID_ERR_ARG, "level-set flow: a median takes width 1 or 2, a Laplacian or mean-curvature flow width 1 (fluid_sdf_set_filter_kind)");
    if (f->grow && !plan::grow_ok(t))
        return fail(FLUID_ERR_ARG, "grown level-set filter: growing the band requires tracking with normalize >= 1 and trim = 1 (fluid_sdf_set_track)");
    if (f->grow && !plan::grown_offset_ok((float)filt->offset, g.dxf))
        return fail(FLUID_ERR_ARG, "grown level-set filter: an offset beyond 4 dx in magnitude is refused");
    if (!f->grow && plan::tracking(t) && !plan::tracked_offset_ok((float)filt->offset, g.bg))
        return fail(FLUID_ERR_ARG, "tracked level-set filter: an offset beyond the background in magnitude leaves no surface");
    f->filt = filt, f->dilate = 4;
    f->attr = false, f->dist2 = false;
    f->tm = nullptr, f->tid = nullptr, f->tvel = nullptr, f->tmin = nullptr;
    const fluid_sdf_surface_t spheres{FLUID_SDF_SURFACE_SPHERES, 0, 0.0};
    const fluid_sdf_surface_t& sf = sf_arg ? *sf_arg : tr_arg ? spheres : s->sdf->surface;   // (trails handed in: spheres and these trails)
    f->record = false;
    f->averaged = sf.kind == FLUID_SDF_SURFACE_AVERAGED;
    const adef::Consts hc = f->averaged ? adef::consts(sf.influence) : adef::Consts{0.0f, 0.0f};
    f->h2 = hc.h2, f->ih2 = hc.ih2;
    f->trails_arg = tr_arg != nullptr;
    f->trails = tr_arg || (!sf_arg && s->sdf->trails_on);   // (a surface handed in is the averaged rank record's: the setting is not read)
    f->tr = tr_arg ? *tr_arg : s->sdf->trails;
    if (f->trails && !tdef::radius_ok(f->tr.radius_min, R))
        return fail(FLUID_ERR_ARG, "velocity trails: radius_min <= radius is required (fluid_sdf_set_trails)");
    return FLUID_OK;
}

int fl::sdf_front(fluid_sim* s, SdfFront* f)
{
    SdfState* o = s->sdf;
    SdfGeom& g = f->g;
    int rc;
    if (f->averaged && f->attr) return fail(FLUID_ERR_STATE, SDF_AVG_ATTR);
    if (f->trails && f->attr) return fail(FLUID_ERR_STATE, SDF_TRAIL_ATTR);
    const Particles live = s->pa.shifted(s->p_off);
    int* box = o->h_small;
    long items = s->np;   // what is binned: the live particles, or their instances
    tdef::Consts tc{};
    // the entries of a decomposed handle that are dead have no instance; the trails handed in keep counters of their own
    const bool tlive = f->trails && s->dist;
    int64_t& t_particles = f->trails_arg ? o->dist_trail_particles : o->trail_particles;
    int64_t& t_instances = f->trails_arg ? o->dist_trail_instances : o->trail_instances;
    if (f->trails) {
        const fluid_sdf_trails_t& t = f->tr;
        tc = tdef::consts(t.shutter, t.delta, t.radius_min, t.max_instances, g.R);
        t_particles = tlive ? 0 : s->np, t_instances = 0;
    }
    if (s->np > 0 && f->trails) {
        if ((rc = trail_scratch(o, s->np, 0))) return rc;
        launch_trail_count(s->st, s->np, live, tc, g.lo, g.hi, o->icnt, o->d_small, tlive);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(o->h_small, o->d_small, 6 * sizeof(int), hipMemcpyDeviceToHost, s->st));
        HIPCHK(hipMemcpyAsync(o->h_small + 8, o->d_small + 8, (tlive ? 4 : 2) * sizeof(int), hipMemcpyDeviceToHost, s->st));
        HIPCHK(hipStreamSynchronize(s->st));
        uint64_t total, alive = (uint64_t)s->np;   // every instance total lies in [live particles, MAX_INSTANCES x live particles]
        memcpy(&total, o->h_small + 8, sizeof total);
        if (tlive) memcpy(&alive, o->h_small + 10, sizeof alive);
        if (alive > (uint64_t)s->np) return fail(FLUID_ERR_HIP, "velocity trails: live count out of range");
        if (total < alive || total > alive * tdef::MAX_INSTANCES) return fail(FLUID_ERR_HIP, "velocity trails: instance total out of range");
        if (total > 0x7fffffffull) return fail(FLUID_ERR_ARG, "velocity trails: more than 2^31 - 1 instances");
        t_particles = (int64_t)alive, t_instances = (int64_t)total;
        items = (long)total;   // (0: nothing live, and the box read back is k_trail_init's empty one)
    } else if (s->np > 0) {
        launch_sdf_bbox(s->st, s->np, live, g.lo, g.hi, o->d_small, s->dist);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(o->h_small, o->d_small, 6 * sizeof(int), hipMemcpyDeviceToHost, s->st));
        HIPCHK(hipStreamSynchronize(s->st));
    }
    if (s->np > 0 && box[3] >= box[0]) {
        for (int a = 0; a < 3; ++a)
            if (box[a] < g.lo || box[3 + a] > g.hi || box[3 + a] < box[a]) return fail(FLUID_ERR_HIP, "level set: particle box out of range");
        g.bx0 = box[0], g.by0 = box[1], g.bz0 = box[2];
        g.bnx = box[3] - box[0] + 1, g.bny = box[4] - box[1] + 1, g.bnz = box[5] - box[2] + 1;
        // T grown tracks move the active set by at most T cells (Manhattan)
        const int dilate = f->dilate + (f->grow ? plan::tracks(*f->filt, g.dxf) : 0);
        for (int a = 0; a < 3; ++a) {
            const int c0 = std::max(box[a] - dilate, g.lo), c1 = std::min(box[3 + a] + dilate, g.hi);
            g.l0[a] = (c0 - g.L0) >> 3;
            g.nl[a] = ((c1 - g.L0) >> 3) - g.l0[a] + 1;
        }
        const long cells = g.cells(), leaves = g.leaves();
        const bool tracked = f->track_n > 0 || f->track_trim;
        if (cells + 1 > 0x7fffffffL || leaves > 0x7fffffffL) return fail(FLUID_ERR_ARG, "level set: the particles' box is too large");
        if ((rc = sdf_scratch(o, cells + 1, items, leaves, f->filt != nullptr, f->attr, f->dist2 || f->record, tracked, f->grow, f->record))) return rc;
        double *sx = o->spos, *sy = o->spos + o->part_cap, *sz = o->spos + 2 * o->part_cap;
        Particles inst{};   // trails: the instances stand where the particles stood (positions only)
        if (f->trails) {
            if ((rc = trail_scratch(o, s->np, items))) return rc;
            inst.px = o->ipos, inst.py = o->ipos + o->inst_cap, inst.pz = o->ipos + 2 * o->inst_cap;
            launch_exclusive_scan(s->st, o->icnt, o->ioff, s->np, o->isums, o->d_small + 6);   // (the total is known; d_small[6] is rewritten below)
            launch_trail_expand(s->st, s->np, live, tc, o->ioff, items, inst.px, inst.py, inst.pz, o->ir, tlive);
        }
        HIPCHK(hipMemsetAsync(o->cnt, 0, (size_t)(cells + 1) * sizeof(int), s->st));
        launch_sdf_count(s->st, items, f->trails ? inst : live, g, o->cnt, o->place, s->dist && !f->trails);   // (the instances have no pid: none is dead)
        launch_exclusive_scan(s->st, o->cnt, o->start, cells + 1, o->cell_sums, o->d_small + 6);   // start[cells] = the counted particles
        if (f->trails) launch_trail_scatter(s->st, items, inst.px, inst.py, inst.pz, o->ir, g, o->start, o->place, sx, sy, sz, o->sr);
        else launch_sdf_scatter(s->st, s->np, live, g, o->start, o->place, sx, sy, sz, f->attr ? o->ssrc : nullptr);
        if (f->trails) launch_sdf_search_rad(s->st, g, o->start, sx, sy, sz, o->sr, o->tv, o->tm, o->flags);
        else if (f->record) launch_sdf_search_avg_record(s->st, g, f->h2, f->ih2, o->start, sx, sy, sz, o->tmin, o->tsum, o->flags);
        else if (f->averaged) launch_sdf_search_avg(s->st, g, f->h2, f->ih2, o->start, sx, sy, sz, o->tv, o->tm, o->flags);
        else if (f->attr) launch_sdf_search_attr(s->st, g, o->start, sx, sy, sz, o->tv, o->tm, o->flags, o->ssrc, live, o->tid, o->tvel, f->dist2 ? o->tmin : nullptr);
        else launch_sdf_search(s->st, g, o->start, sx, sy, sz, o->tv, o->tm, o->flags, o->count_visits ? o->visits : nullptr);
        f->any = true;
        f->tv = o->tv, f->flags = o->flags, f->list = o->flags;
        f->tm = o->tm;
        if (f->attr) f->tid = o->tid, f->tvel = o->tvel;
        if (f->dist2 || f->record) f->tmin = o->tmin;
        if (f->filt) {
            // the schedule of passes, offset steps and tracks: sdf_filter_plan.h; here what each of them launches
            float *src = o->tv, *dst = o->tv2;
            int *flags = o->flags, *flags2 = o->flags2;   // grown: the dilation's ping-pong
            uint64_t *tm = o->tm, *tm2 = o->tm2;
            const long flagged0 = o->grow_stats && tracked ? sdf_count_flags(s, o->flags, leaves) : 0;
            bool trimmed = false;
            plan::run(
                f->kind, *f->filt, g.dxf, tracked,
                [&](int axis, int W, float off) {
                    launch_sdf_box(s->st, g, axis, W, off, flags, tm, src, dst);
                    std::swap(src, dst);
                },
                [&](int kind, int W, float off) {
                    launch_sdf_flow(s->st, g, kind, W, off, flags, tm, src, dst);
                    std::swap(src, dst);
                },
                [&](float step) { launch_sdf_offset(s->st, g, step, flags, tm, src); },
                [&]() {   // one track: N passes src -> dst, the trim on the last; without a pass the trim alone, in place
                    if (f->grow) {   // a newly flagged leaf gets its +bg in src, which the first pass below reads
                        launch_sdf_grow(s->st, g, flags, tm, flags2, tm2, src, f->attr ? o->tid : nullptr, o->tvel);
                        std::swap(flags, flags2), std::swap(tm, tm2);
                    }
                    for (int i = 0; i < f->track_n; ++i) {
                        const bool last = i == f->track_n - 1;
                        uint32_t* tid = f->attr ? o->tid : nullptr;
                        if (f->track_scheme == FLUID_SDF_TRACK_HJWENO5) launch_sdf_track_weno(s->st, g, last && f->track_trim, flags, tm, src, dst, tid, o->tvel);
                        else launch_sdf_track(s->st, g, true, last && f->track_trim, flags, tm, src, dst, tid, o->tvel);
                        std::swap(src, dst);
                    }
                    if (f->track_n == 0) launch_sdf_track(s->st, g, false, true, flags, tm, src, src, f->attr ? o->tid : nullptr, o->tvel);
                    trimmed = f->track_trim;
                });
            if (trimmed) launch_sdf_relist(s->st, g, flags, tm, src, o->lflags);   // what is listed is what the last trim left
            f->list = trimmed ? o->lflags : flags;
            f->flags = flags, f->tm = tm, f->tv = src;
            if (o->grow_stats && tracked) {
                const size_t per_leaf = 2 * 2048 + 64 + 3 * sizeof(int) + (o->tracked ? sizeof(int) : 0) + (o->grown ? 64 + sizeof(int) : 0) +
                                        (o->attr ? 2048 + 6144 : 0) + (o->dist2 ? 2048 : 0);
                fprintf(stderr, "sdf grow: grow %d leaves_in_range %ld flagged_by_search %ld flagged_at_end %ld leaf_scratch_bytes %zu\n", f->grow ? 1 : 0, leaves,
                        flagged0, sdf_count_flags(s, flags, leaves), (size_t)o->leaf_cap * per_leaf);
            }
        }
    }
    return FLUID_OK;
}

// front half -> scan of the flags -> pack -> copy
static constexpr size_t sdf_rec(int kind)   // bytes per listed leaf of a record: plain, with attributes, with attributes and dist2, averaged rank record
{
    if (kind == SDF_AVG_RECORD) return FLUID_SDF_AVG_PART_LEAF_BYTES;   // (the longest of the four: `wide` stays ordered)
    return SDF_REC + (kind >= 1 ? (size_t)FLUID_SDF_ATTR_LEAF_BYTES : 0) + (kind >= 2 ? (size_t)2048 : 0);
}
static constexpr size_t sdf_between(int kind) { return sdf_rec(kind) - SDF_REC; }   // per leaf, between the values and the masks

static int sdf_capture(fluid_sim* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* filt = nullptr, int attr = 0,
                       const fluid_sdf_surface_t* sf = nullptr, const fluid_sdf_trails_t* tr = nullptr)
{
    SdfFront f;
    int rc = sdf_begin(s, p, &f, filt, sf, tr);
    if (rc) return rc;
    const bool record = attr == SDF_AVG_RECORD;
    f.attr = attr >= 1 && !record, f.dist2 = attr == 2, f.record = record;
    SdfState* o = s->sdf;
    if (snap_full(o->ring)) return fail(FLUID_ERR_STATE, "two level-set snapshots are waiting for fluid_sdf_wait");
    SnapSlot& q = o->ring.s[snap_slot(o->ring)];
    SdfMeta& m = o->m[snap_slot(o->ring)];
    if ((rc = sdf_front(s, &f))) return rc;
    const SdfGeom& g = f.g;
    const float R = g.R, w = g.w;
    int n = 0;
    if (f.any) {
        const long leaves = g.leaves();
        launch_exclusive_scan(s->st, f.list, o->slot, leaves, o->leaf_sums, o->d_small + 7);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(o->h_small + 7, o->d_small + 7, sizeof(int), hipMemcpyDeviceToHost, s->st));
        HIPCHK(hipStreamSynchronize(s->st));
        n = o->h_small[7];
        if (n < 0 || (long)n > leaves) return fail(FLUID_ERR_HIP, "level set: leaf count out of range");
        if (o->count_visits && !attr) {   // cells looked at and voxels computed, for tools/sdf_cost.py
            std::vector<unsigned> v((size_t)leaves);
            HIPCHK(hipMemcpy(v.data(), o->visits, (size_t)leaves * sizeof(unsigned), hipMemcpyDeviceToHost));
            double cv = 0;
            long searched = 0;
            for (long j = 0; j < leaves; ++j) cv += v[(size_t)j], searched += v[(size_t)j] > 0;
            fprintf(stderr, "sdf visits: cells %.0f leaves_searched %ld leaves_in_range %ld\n", cv, searched, leaves);
        }
    }
    if (attr > m.wide) m.wide = attr;   // (and stays so)
    if ((rc = snap_reserve(q, (size_t)n * sdf_rec(m.wide), 64 * sdf_rec(m.wide)))) return rc;
    m.n_leaves = n;
    m.attr = attr;
    const size_t rec = sdf_rec(attr);
    m.bg = g.bg, m.R = R, m.w = w;
    m.dxf = g.dxf, m.hf = record ? (float)sf->influence : 0.0f;
    if (n > 0 && record) {
        launch_sdf_pack_avg(s->st, g, f.list, o->slot, f.tmin, o->tsum, (float*)q.dev, (uint64_t*)(q.dev + (size_t)n * 2048),
                            (int*)(q.dev + (size_t)n * (2048 + 16384)));
        HIPCHK(hipGetLastError());
    } else if (n > 0) {
        const size_t a = (size_t)n * sdf_between(attr);   // the attributes lie between the values and the masks
        float* values = (float*)q.dev;
        uint64_t* active = (uint64_t*)(q.dev + (size_t)n * 2048 + a);
        int* origin = (int*)(q.dev + (size_t)n * (2048 + 64) + a);
        if (attr)
            launch_sdf_pack_attr(s->st, g, f.list, o->slot, f.tv, f.tm, values, active, origin, f.tid, f.tvel, (uint32_t*)(q.dev + (size_t)n * 2048),
                                 (float*)(q.dev + (size_t)n * 4096), f.tmin, attr >= 2 ? (float*)(q.dev + (size_t)n * 10240) : nullptr);
        else launch_sdf_pack(s->st, g, f.list, o->slot, f.tv, f.tm, values, active, origin);
        HIPCHK(hipGetLastError());
    }
    if ((rc = snap_commit(o->ring, s->st, (size_t)n * rec))) return rc;
    o->last_leaves = n;
    o->last_bytes = (long)((size_t)n * rec) + 4;
    return FLUID_OK;
}

// The oldest outstanding snapshot is (avg) / is not (!avg) an averaged rank record, or there is none: FLUID_OK.  Asked before
// snap_next_wait, so that a refused wait leaves the snapshot outstanding.
static int sdf_wait_kind(const SdfState* o, bool avg)
{
    if (!o || o->ring.n_wait >= o->ring.n_snap) return FLUID_OK;
    const bool is = o->m[o->ring.n_wait & 1].attr == SDF_AVG_RECORD;
    if (is == avg) return FLUID_OK;
    return fail(FLUID_ERR_STATE, avg ? "the oldest level-set snapshot is no averaged rank record: fluid_dist_sdf_wait_avg takes those of fluid_dist_sdf_snapshot_avg alone"
                                     : "the oldest level-set snapshot is an averaged rank record, which holds no values: fluid_dist_sdf_wait_avg takes it");
}

static int sdf_wait(fluid_sim* s, fluid_sdf_grid_t* out, fluid_sdf_attr_t* at = nullptr, fluid_sdf_attr_part_t* part = nullptr)
{
    if (!out) return fail(FLUID_ERR_ARG, "null argument");
    SdfState* o = s->sdf;
    if (int rk = sdf_wait_kind(o, false)) return rk;
    int k = -1, rc = o ? snap_next_wait(o->ring, &k) : FLUID_OK;
    if (rc) return rc;
    if (k < 0) return fail(FLUID_ERR_STATE, "no level-set snapshot is outstanding");
    const char* host = o->ring.s[k].host;
    const SdfMeta& m = o->m[k];
    const size_t n = (size_t)m.n_leaves;
    out->n = s->g.N;
    out->n_leaves = m.n_leaves;
    out->background = m.bg;
    out->radius = m.R;
    out->half_width = m.w;
    out->values = n ? (const float*)host : nullptr;
    const size_t a = n * sdf_between(m.attr);
    out->active = n ? (const uint64_t*)(host + n * 2048 + a) : nullptr;
    out->origin = n ? (const int32_t*)(host + n * (2048 + 64) + a) : nullptr;
    if (at) {
        at->n_leaves = m.n_leaves;
        at->id = n && m.attr ? (const uint32_t*)(host + n * 2048) : nullptr;
        at->velocity = n && m.attr ? (const float*)(host + n * 4096) : nullptr;
    }
    if (part) {   // a record of a rank: only a snapshot that carries dist2 has one
        const bool has = n && m.attr >= 2;
        part->n_leaves = m.n_leaves;
        part->id = has ? (const uint32_t*)(host + n * 2048) : nullptr;
        part->velocity = has ? (const float*)(host + n * 4096) : nullptr;
        part->dist2 = has ? (const float*)(host + n * 10240) : nullptr;
    }
    return FLUID_OK;
}

static int sdf_wait_avg(fluid_sim* s, fluid_sdf_avg_part_t* out)
{
    if (!out) return fail(FLUID_ERR_ARG, "null argument");
    SdfState* o = s->sdf;
    if (int rk = sdf_wait_kind(o, true)) return rk;
    int k = -1, rc = o ? snap_next_wait(o->ring, &k) : FLUID_OK;
    if (rc) return rc;
    if (k < 0) return fail(FLUID_ERR_STATE, "no level-set snapshot is outstanding");
    const char* host = o->ring.s[k].host;
    const SdfMeta& m = o->m[k];
    const size_t n = (size_t)m.n_leaves;
    out->n = s->g.N;
    out->n_leaves = m.n_leaves;
    out->background = m.bg, out->radius = m.R, out->half_width = m.w, out->dx = m.dxf, out->influence = m.hf;
    out->dist2 = n ? (const float*)host : nullptr;
    out->sums = n ? (const uint64_t*)(host + n * 2048) : nullptr;
    out->origin = n ? (const int32_t*)(host + n * (2048 + 16384)) : nullptr;
    return FLUID_OK;
}

static int sdf_stats(fluid_sim* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host)
{
    const int64_t nl = grid_leaves(s->g);
    if (leaves_in_grid) *leaves_in_grid = nl * nl * nl;
    if (leaves_listed) *leaves_listed = s->sdf ? s->sdf->last_leaves : 0;
    if (bytes_to_host) *bytes_to_host = s->sdf ? s->sdf->last_bytes : 0;
    return FLUID_OK;
}

static bool sdf_averaged(const fluid_sim* s) { return s->sdf && s->sdf->surface.kind == FLUID_SDF_SURFACE_AVERAGED; }
static bool sdf_trails(const fluid_sim* s) { return s->sdf && s->sdf->trails_on; }

void fl::sdf_move(fluid_sim* from, fluid_sim* to)
{
    sdf_free(to);
    to->sdf = from->sdf;
    from->sdf = nullptr;
}

extern "C" {

int fluid_sdf_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p)
{
    int rc = snap_guard(s, SDF_SINGLE);
    return rc ? rc : sdf_capture(s, p);
}

int fluid_sdf_snapshot_filtered(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f)
{
    if (int rc = snap_guard(s, SDF_FILT_SINGLE)) return rc;
    if (!f) return fail(FLUID_ERR_ARG, "null argument");
    return sdf_capture(s, p, f);
}

int fluid_sdf_set_track(fluid_sim_t* s, const fluid_sdf_track_t* t)
{
    if (int rc = snap_guard(s, SDF_TRACK_SINGLE)) return rc;
    if (!plan::track_ok(t))
        return fail(FLUID_ERR_ARG, "level-set tracking: normalize in 0..8, trim 0 or 1 and scheme FLUID_SDF_TRACK_FIRST_BIAS or FLUID_SDF_TRACK_HJWENO5 are required");
    HIPCHK(hipSetDevice(s->prm.device));
    if (int rc = sdf_init(s)) return rc;
    s->sdf->track = t ? *t : fluid_sdf_track_t{0, 0, FLUID_SDF_TRACK_FIRST_BIAS};
    return FLUID_OK;
}

int fluid_sdf_set_track_grow(fluid_sim_t* s, int32_t grow)
{
    if (int rc = snap_guard(s, SDF_GROW_SINGLE)) return rc;
    if (grow != 0 && grow != 1) return fail(FLUID_ERR_ARG, "level-set tracking: grow is 0 or 1");
    HIPCHK(hipSetDevice(s->prm.device));
    if (int rc = sdf_init(s)) return rc;
    s->sdf->track_grow = grow != 0;
    return FLUID_OK;
}

int fluid_sdf_set_filter_kind(fluid_sim_t* s, int32_t kind)
{
    if (int rc = snap_guard(s, SDF_KIND_SINGLE)) return rc;
    if (!plan::kind_ok(kind)) return fail(FLUID_ERR_ARG, "level-set filter kind: one of FLUID_SDF_FILTER_BOX, _MEDIAN, _LAPLACIAN, _MEAN_CURVATURE is required");
    HIPCHK(hipSetDevice(s->prm.device));
    if (int rc = sdf_init(s)) return rc;
    s->sdf->kind = kind;
    return FLUID_OK;
}

int fluid_sdf_set_surface(fluid_sim_t* s, const fluid_sdf_surface_t* sf)
{
    if (int rc = snap_guard(s, SDF_AVG_SINGLE)) return rc;
    if (sf && sf->kind != FLUID_SDF_SURFACE_SPHERES) {
        if (sf->kind != FLUID_SDF_SURFACE_AVERAGED || sf->reserved != 0 || !adef::influence_ok(sf->influence))
            return fail(FLUID_ERR_ARG, "level-set surface: kind FLUID_SDF_SURFACE_SPHERES or _AVERAGED, reserved 0 and 0 < influence <= 4 (voxels) are required");
    }
    const bool avg = sf && sf->kind == FLUID_SDF_SURFACE_AVERAGED;
    if (avg && sdf_trails(s)) return fail(FLUID_ERR_STATE, SDF_TRAIL_AVG);
    HIPCHK(hipSetDevice(s->prm.device));
    if (int rc = sdf_init(s)) return rc;
    s->sdf->surface = avg ? *sf : fluid_sdf_surface_t{FLUID_SDF_SURFACE_SPHERES, 0, 0.0};
    return FLUID_OK;
}

int fluid_sdf_set_trails(fluid_sim_t* s, const fluid_sdf_trails_t* t)
{
    if (int rc = snap_guard(s, SDF_TRAIL_SINGLE)) return rc;
    if (t && !tdef::settings_ok(t->shutter, t->delta, t->radius_min, t->max_instances, t->reserved))
        return fail(FLUID_ERR_ARG, "velocity trails: a finite shutter >= 0, delta > 0 and radius_min > 0 (voxels), max_instances in 1..32 and reserved 0 are required");
    if (t && sdf_averaged(s)) return fail(FLUID_ERR_STATE, SDF_TRAIL_AVG);
    HIPCHK(hipSetDevice(s->prm.device));
    if (int rc = sdf_init(s)) return rc;
    s->sdf->trails_on = t != nullptr;
    s->sdf->trails = t ? *t : fluid_sdf_trails_t{0.0, 0.0, 0.0, 0, 0};
    return FLUID_OK;
}

int fluid_sdf_trails_stats(fluid_sim_t* s, int64_t* particles, int64_t* instances)
{
    if (int rc = snap_guard(s, SDF_TRAIL_SINGLE)) return rc;
    if (particles) *particles = s->sdf ? s->sdf->trail_particles : 0;
    if (instances) *instances = s->sdf ? s->sdf->trail_instances : 0;
    return FLUID_OK;
}

int fluid_sdf_wait(fluid_sim_t* s, fluid_sdf_grid_t* out)
{
    int rc = snap_guard(s, SDF_SINGLE);
    return rc ? rc : sdf_wait(s, out);
}

int fluid_sdf_snapshot_attr(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f)
{
    int rc = snap_guard(s, ATTR_SINGLE);
    return rc ? rc : sdf_capture(s, p, f, 1);
}

int fluid_sdf_wait_attr(fluid_sim_t* s, fluid_sdf_grid_t* out, fluid_sdf_attr_t* attr)
{
    int rc = snap_guard(s, ATTR_SINGLE);
    return rc ? rc : sdf_wait(s, out, attr);
}

int fluid_sdf_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host)
{
    int rc = snap_guard(s, SDF_SINGLE);
    return rc ? rc : sdf_stats(s, leaves_in_grid, leaves_listed, bytes_to_host);
}

int fluid_dist_sdf_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    if (sdf_averaged(s)) return fail(FLUID_ERR_STATE, SDF_AVG_DIST);
    if (sdf_trails(s)) return fail(FLUID_ERR_STATE, SDF_TRAIL_DIST);
    return sdf_capture(s, p);
}

int fluid_dist_sdf_wait(fluid_sim_t* s, fluid_sdf_grid_t* out)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    return sdf_wait(s, out);
}

int fluid_dist_sdf_snapshot_attr(fluid_sim_t* s, const fluid_sdf_params_t* p)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    if (sdf_averaged(s)) return fail(FLUID_ERR_STATE, SDF_AVG_DIST);
    if (sdf_trails(s)) return fail(FLUID_ERR_STATE, SDF_TRAIL_DIST);
    return sdf_capture(s, p, nullptr, 2);
}

int fluid_dist_sdf_wait_attr(fluid_sim_t* s, fluid_sdf_grid_t* out, fluid_sdf_attr_part_t* part)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    return sdf_wait(s, out, nullptr, part);
}

int fluid_dist_sdf_snapshot_avg(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_surface_t* sf)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    if (!sf || sf->kind != FLUID_SDF_SURFACE_AVERAGED || sf->reserved != 0 || !adef::influence_ok(sf->influence))
        return fail(FLUID_ERR_ARG, "averaged rank record: kind FLUID_SDF_SURFACE_AVERAGED, reserved 0 and 0 < influence <= 4 (voxels) are required");
    return sdf_capture(s, p, nullptr, SDF_AVG_RECORD, sf);
}

int fluid_dist_sdf_wait_avg(fluid_sim_t* s, fluid_sdf_avg_part_t* out)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    return sdf_wait_avg(s, out);
}

int fluid_dist_sdf_snapshot_trails(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_trails_t* t)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    if (!t || !tdef::settings_ok(t->shutter, t->delta, t->radius_min, t->max_instances, t->reserved))
        return fail(FLUID_ERR_ARG, "trails' rank record: a finite shutter >= 0, delta > 0 and radius_min > 0 (voxels), max_instances in 1..32 and reserved 0 are required");
    return sdf_capture(s, p, nullptr, 0, nullptr, t);
}

int fluid_dist_sdf_trails_stats(fluid_sim_t* s, int64_t* particles, int64_t* instances)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    if (particles) *particles = s->sdf ? s->sdf->dist_trail_particles : 0;
    if (instances) *instances = s->sdf ? s->sdf->dist_trail_instances : 0;
    return FLUID_OK;
}

int fluid_dist_sdf_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host)
{
    if (!s) return fail(FLUID_ERR_ARG, "null handle");
    return sdf_stats(s, leaves_in_grid, leaves_listed, bytes_to_host);
}

}  // extern "C"
