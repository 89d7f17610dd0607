// Mesh snapshots of the liquid surface (include/fluid_hip.h, "liquid surface as a mesh"): the surface nets of the particles' level
// set leave the device as vertices and quads.  Kernels in kernels_mesh.hip.
//
// fluid_mesh_snapshot, all on the handle's stream: the front half of a level-set snapshot (fluid_sdf.hip: bbox, 24 bytes read back,
// count, scan, scatter, search — the search scratch is the surface's own, shared in stream order) -> mark (mask, vertex and quad
// count per leaf of the range) and the two totals (read back: 8 bytes, they size the slot) -> two exclusive scans of the counts ->
// emit into the slot's device staging ([nq x 16 B of quads | nv x 12 B of vertices]); the records then leave through the mesh's own
// ring of two slots (snap_ring.h).  No leaf is packed.  The particle arrays are only read and `binned` keeps holding, as for the
// surface.
//
// fluid_mesh_snapshot_filtered ("liquid surface, smoothed"): the front half runs over the box dilated by 5 cells and ends with the
// filter's box passes (fluid_sdf.hip); the mesh kernels read the buffer the last pass wrote.  After the filter an inside voxel is
// only known to be active or -bg, so within 4 cells of a base cell, and a mixed cell's min corner within [-5, +4]: kernels_mesh.hip's
// range argument with every distance one larger.
//
// fluid_mesh_snapshot_attr ("liquid surface, attributes"): the front half's search also leaves the closest particle's velocity per
// voxel, the emit kernel writes a velocity per vertex, and the slot's record is [quads | vertices | nv x 12 B of velocities].
//
// fluid_mesh_snapshot_ex ("normals and triangles"): `what` chooses velocities, normals and triangles; the record is
// [quads | nq x 24 B of triangles | vertices | velocities | normals], each part only if asked for.  The triangles sit right behind
// the quads so that they start at a multiple of 16 for every nv and nq (behind the vertices 12 nv would leave 4); k_mesh_tris runs
// behind emit on the handle's stream.  what = 0 and 1 give the records above byte for byte.
#include "sim.h"

using namespace fl;
#define fail fluid_fail

struct MeshMeta {              // per slot of the ring
    long nv = 0, nq = 0;
    unsigned what = 0;         // FLUID_MESH_* bits: what the snapshot in the slot carries beside vertices and quads
    size_t tris_at() const { return (size_t)nq * 16; }
    size_t vert_at() const { return (size_t)nq * ((what & FLUID_MESH_TRIANGLES) ? 40 : 16); }
    size_t vel_at() const { return vert_at() + (size_t)nv * 12; }
    size_t nrm_at() const { return vel_at() + ((what & FLUID_MESH_VELOCITY) ? (size_t)nv * 12 : 0); }
    size_t bytes() const { return nrm_at() + ((what & FLUID_MESH_NORMALS) ? (size_t)nv * 12 : 0); }
    float bg = 0, R = 0, w = 0;
};
struct MeshState {
    long leaf_cap = 0;            // leaves of the range the per-leaf scratch holds
    uint64_t* cmask = nullptr;    // 8 words per leaf
    int *cpre = nullptr, *vcnt = nullptr, *qcnt = nullptr, *vbase = nullptr, *qbase = nullptr, *sums = nullptr;
    int* d_scan_tot = nullptr;    // where launch_exclusive_scan puts its 32-bit totals (it always writes one; d_tot is what is read)
    unsigned *d_tot = nullptr, *h_tot = nullptr;   // vertices, quads: saturating at 2^31
    SnapRing ring;
    MeshMeta m[2];
    long last_v = 0, last_q = 0;
    unsigned last_what = 0;
};

static const char* const MESH_SINGLE = "mesh snapshots are single-GPU only: a decomposed run merges its blocks' level-set lists (fluid_sdf_grids_merge) and meshes the result on the host (fluid_sdf_mesh)";
static const char* const MESH_EX_SINGLE = "mesh snapshots with normals or triangles are single-GPU only: a decomposed run merges its blocks' level-set lists (fluid_sdf_grids_merge), meshes the result on the host (fluid_sdf_mesh) and adds fluid_sdf_mesh_normals and fluid_mesh_triangles";
static const char* const MESH_FILT_SINGLE = "filtered mesh snapshots are single-GPU only: a decomposed run merges its blocks' level-set lists (fluid_sdf_grids_merge), filters the result (fluid_sdf_filter) and meshes it on the host (fluid_sdf_mesh)";

static int mesh_init(fluid_sim* s)
{
    if (s->mesh) return FLUID_OK;
    MeshState* o = new MeshState();
    s->mesh = o;   // from here on mesh_free releases whatever the lines below got
    HIPCHK(hipMalloc((void**)&o->d_tot, 2 * sizeof(unsigned)));
    HIPCHK(hipMalloc((void**)&o->d_scan_tot, 2 * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&o->h_tot, 2 * sizeof(unsigned)));
    return snap_init(o->ring);
}

void fl::mesh_free(fluid_sim* s)
{
    MeshState* o = s->mesh;
    if (!o) return;
    snap_free(o->ring);
    for (void* p : {(void*)o->cmask, (void*)o->cpre, (void*)o->vcnt, (void*)o->qcnt, (void*)o->vbase, (void*)o->qbase, (void*)o->sums,
                    (void*)o->d_scan_tot, (void*)o->d_tot})
        if (p) hipFree(p);
    if (o->h_tot) hipHostFree(o->h_tot);
    delete o;
    s->mesh = nullptr;
}

// (the front half's kernels are still queued on the handle's stream here; none of them touches these buffers, the mesh kernels
// of the snapshot before have ended — the front half waited for the box behind them — and hipFree waits for the device anyway)
static int mesh_scratch(MeshState* o, long leaves)
{
    if (leaves <= o->leaf_cap) return FLUID_OK;
    o->leaf_cap = 0;
    const long cap = leaves + leaves / 4 + 64;
    HIPCHK(regrow(o->cmask, (size_t)cap * 8));
    HIPCHK(regrow(o->cpre, (size_t)cap * 8));
    HIPCHK(regrow(o->vcnt, (size_t)cap));
    HIPCHK(regrow(o->qcnt, (size_t)cap));
    HIPCHK(regrow(o->vbase, (size_t)cap));
    HIPCHK(regrow(o->qbase, (size_t)cap));
    HIPCHK(regrow(o->sums, (size_t)cap / 2048 + 16));
    o->leaf_cap = cap;
    return FLUID_OK;
}

static int mesh_capture(fluid_sim* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* filt, unsigned what = 0)
{
    const bool attr = (what & FLUID_MESH_VELOCITY) != 0;
    SdfFront f;
    int rc = sdf_begin(s, p, &f, filt);
    if (rc) return rc;
    if (filt) f.dilate = 5;
    f.attr = attr;
    if ((rc = mesh_init(s))) return rc;
    MeshState* o = s->mesh;
    if (snap_full(o->ring)) return fail(FLUID_ERR_STATE, "two mesh snapshots are waiting for fluid_mesh_wait");
    SnapSlot& q = o->ring.s[snap_slot(o->ring)];
    MeshMeta& m = o->m[snap_slot(o->ring)];
    if ((rc = sdf_front(s, &f))) return rc;
    const SdfGeom& g = f.g;
    long nv = 0, nq = 0;
    if (f.any) {
        const long leaves = g.leaves();
        if ((rc = mesh_scratch(o, leaves))) return rc;
        launch_mesh_mark(s->st, g, f.tv, f.flags, o->cmask, o->cpre, o->vcnt, o->qcnt, o->d_tot);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(o->h_tot, o->d_tot, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s->st));
        launch_exclusive_scan(s->st, o->vcnt, o->vbase, leaves, o->sums, o->d_scan_tot);
        launch_exclusive_scan(s->st, o->qcnt, o->qbase, leaves, o->sums, o->d_scan_tot + 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->st));
        if (o->h_tot[0] > 0x7fffffffu || o->h_tot[1] > 0x7fffffffu)
            return fail(FLUID_ERR_ARG, "mesh: more than 2^31 - 1 vertices or quads");
        nv = (long)o->h_tot[0], nq = (long)o->h_tot[1];
    }
    MeshMeta nm;
    nm.nv = nv, nm.nq = nq;
    nm.what = what;
    nm.bg = g.bg, nm.R = g.R, nm.w = g.w;
    const size_t bytes = nm.bytes();
    if ((rc = snap_reserve(q, bytes, 4096))) return rc;
    m = nm;
    if (nv > 0) {
        float* const vert = (float*)(q.dev + m.vert_at());
        launch_mesh_emit(s->st, g, f.tv, f.flags, attr ? f.tm : nullptr, attr ? f.tvel : nullptr, o->cmask, o->cpre, o->vcnt, o->qcnt, o->vbase, o->qbase,
                         vert, (uint32_t*)q.dev, attr ? (float*)(q.dev + m.vel_at()) : nullptr,
                         (what & FLUID_MESH_NORMALS) ? (float*)(q.dev + m.nrm_at()) : nullptr);
        if (what & FLUID_MESH_TRIANGLES) launch_mesh_tris(s->st, nq, nv, (const uint32_t*)q.dev, vert, (uint32_t*)(q.dev + m.tris_at()));
        HIPCHK(hipGetLastError());
    }
    if ((rc = snap_commit(o->ring, s->st, nv > 0 ? bytes : 0))) return rc;
    o->last_v = nv, o->last_q = nq;
    o->last_what = what;
    return FLUID_OK;
}

static int mesh_wait(fluid_sim* s, fluid_mesh_t* out, fluid_mesh_attr_t* at, fluid_mesh_ex_t* ex = nullptr)
{
    if (!out) return fail(FLUID_ERR_ARG, "null argument");
    MeshState* o = s->mesh;
    int k = -1, rc = o ? snap_next_wait(o->ring, &k) : FLUID_OK;
    if (rc) return rc;
    if (k < 0) return fail(FLUID_ERR_STATE, "no mesh snapshot is outstanding");
    const char* host = o->ring.s[k].host;
    const MeshMeta& m = o->m[k];
    out->n = s->g.N;
    out->n_vertices = m.nv;
    out->n_quads = m.nq;
    out->radius = m.R;
    out->half_width = m.w;
    out->background = m.bg;
    out->quads = m.nq ? (const uint32_t*)host : nullptr;
    out->vertices = m.nv ? (const float*)(host + m.vert_at()) : nullptr;
    const float* const vel = m.nv && (m.what & FLUID_MESH_VELOCITY) ? (const float*)(host + m.vel_at()) : nullptr;
    if (at) {
        at->n_vertices = m.nv;
        at->velocity = vel;
    }
    if (ex) {
        const bool tris = m.nq && (m.what & FLUID_MESH_TRIANGLES);
        ex->velocity = vel;
        ex->normals = m.nv && (m.what & FLUID_MESH_NORMALS) ? (const float*)(host + m.nrm_at()) : nullptr;
        ex->triangles = tris ? (const uint32_t*)(host + m.tris_at()) : nullptr;
        ex->n_triangles = tris ? 2 * m.nq : 0;
    }
    return FLUID_OK;
}

extern "C" {

int fluid_mesh_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p)
{
    int rc = snap_guard(s, MESH_SINGLE);
    return rc ? rc : mesh_capture(s, p, nullptr);
}

int fluid_mesh_snapshot_filtered(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f)
{
    if (int rc = snap_guard(s, MESH_FILT_SINGLE)) return rc;
    if (!f) return fail(FLUID_ERR_ARG, "null argument");
    return mesh_capture(s, p, f);
}

int fluid_mesh_wait(fluid_sim_t* s, fluid_mesh_t* out)
{
    int rc = snap_guard(s, MESH_SINGLE);
    return rc ? rc : mesh_wait(s, out, nullptr);
}

int fluid_mesh_snapshot_attr(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f)
{
    int rc = snap_guard(s, ATTR_SINGLE);
    return rc ? rc : mesh_capture(s, p, f, FLUID_MESH_VELOCITY);
}

int fluid_mesh_wait_attr(fluid_sim_t* s, fluid_mesh_t* out, fluid_mesh_attr_t* attr)
{
    int rc = snap_guard(s, ATTR_SINGLE);
    return rc ? rc : mesh_wait(s, out, attr);
}

int fluid_mesh_snapshot_ex(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f, uint32_t what)
{
    if (int rc = snap_guard(s, MESH_EX_SINGLE)) return rc;
    if (what & ~(FLUID_MESH_VELOCITY | FLUID_MESH_NORMALS | FLUID_MESH_TRIANGLES)) return fail(FLUID_ERR_ARG, "fluid_mesh_snapshot_ex: unknown bits in `what`");
    return mesh_capture(s, p, f, what);
}

int fluid_mesh_wait_ex(fluid_sim_t* s, fluid_mesh_t* out, fluid_mesh_ex_t* ex)
{
    int rc = snap_guard(s, MESH_EX_SINGLE);
    return rc ? rc : mesh_wait(s, out, nullptr, ex);
}

int fluid_mesh_stats(fluid_sim_t* s, int64_t* vertices, int64_t* quads, int64_t* bytes_to_host)
{
    if (int rc = snap_guard(s, MESH_SINGLE)) return rc;
    const int64_t nv = s->mesh ? s->mesh->last_v : 0, nq = s->mesh ? s->mesh->last_q : 0;
    if (vertices) *vertices = nv;
    if (quads) *quads = nq;
    if (bytes_to_host) {
        MeshMeta m;
        m.nv = nv, m.nq = nq;
        m.what = s->mesh ? s->mesh->last_what : 0;
        *bytes_to_host = s->mesh ? (int64_t)m.bytes() + 8 : 0;
    }
    return FLUID_OK;
}

}  // extern "C"
