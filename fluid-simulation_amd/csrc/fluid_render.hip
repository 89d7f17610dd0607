// Images of the liquid surface (include/fluid_hip.h, "liquid surface as an image"): the particles' level set is ray-cast on the
// device and leaves it as pixels.  Kernels in kernels_render.hip.
//
// fluid_render_snapshot, all on the handle's stream: the front half of a level-set snapshot (fluid_sdf.hip: bbox, 24 bytes read back,
// count, scan, scatter, search, with a filter its box passes over the box dilated by 5 — fluid_mesh.hip's argument: after the filter
// a negative voxel is only known to be active or -bg) -> 16 bytes of header zeroed in the slot's device staging -> neg, occ, march,
// which writes [header: hits | rgb, padded to 16 | depth | normals], each part only if asked for; the record then leaves through the
// image's own ring of two slots (snap_ring.h).  No leaf is packed and nothing is read back beyond the front half's box: the hit count
// is the record's first word.  The particle arrays are only read and `binned` keeps holding, as for the surface.
#include "sim.h"
#include "render_def.h"

using namespace fl;
#define fail fluid_fail

struct RenderMeta {   // per slot of the ring
    int width = 0, height = 0;
    unsigned what = 0;
};
struct RenderState {
    long leaf_cap = 0, word_cap = 0;   // leaves of the range `neg` holds, words of the extended range `occ` holds
    unsigned char* neg = nullptr;
    unsigned* occ = nullptr;
    SnapRing ring;
    RenderMeta m[2];
    long last_px = 0, last_hits = 0;
    unsigned last_what = 0;
};

static const char* const RENDER_SINGLE = "render snapshots are single-GPU only: a decomposed run merges its blocks' level-set lists (fluid_sdf_grids_merge), filters the result if it likes (fluid_sdf_filter) and renders it on the host (fluid_sdf_render)";

static int render_init(fluid_sim* s)
{
    if (s->render) return FLUID_OK;
    s->render = new RenderState();   // from here on render_free releases whatever there is
    return snap_init(s->render->ring);
}

void fl::render_free(fluid_sim* s)
{
    RenderState* o = s->render;
    if (!o) return;
    snap_free(o->ring);
    if (o->neg) hipFree(o->neg);
    if (o->occ) hipFree(o->occ);
    delete o;
    s->render = nullptr;
}

// (the front half's kernels may still be queued on the handle's stream: none of them touches these buffers, and hipFree waits for
// the device)
static int render_scratch(RenderState* o, long leaves, long words)
{
    if (leaves > o->leaf_cap) {
        o->leaf_cap = 0;
        const long cap = leaves + leaves / 4 + 64;
        HIPCHK(regrow(o->neg, (size_t)cap));
        o->leaf_cap = cap;
    }
    if (words > o->word_cap) {
        o->word_cap = 0;
        const long cap = words + words / 4 + 64;
        HIPCHK(regrow(o->occ, (size_t)cap));
        o->word_cap = cap;
    }
    return FLUID_OK;
}

extern "C" {

int fluid_render_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* filt, const fluid_camera_t* cam,
                          const fluid_shade_t* shade, uint32_t what)
{
    int rc = snap_guard(s, RENDER_SINGLE);
    if (rc) return rc;
    if (const char* why = rdef::check(cam, shade, what)) return fail(FLUID_ERR_ARG, why);
    SdfFront f;
    if ((rc = sdf_begin(s, p, &f, filt))) return rc;
    if (filt) f.dilate = 5;
    if ((rc = render_init(s))) return rc;
    RenderState* o = s->render;
    if (snap_full(o->ring)) return fail(FLUID_ERR_STATE, "two render snapshots are waiting for fluid_render_wait");
    const int k = snap_slot(o->ring);
    SnapSlot& q = o->ring.s[k];
    if ((rc = sdf_front(s, &f))) return rc;
    RenderGeom r{};
    r.g = f.g;
    r.any = f.any ? 1 : 0;
    if (f.any) {
        const SdfGeom& g = f.g;
        for (int a = 0; a < 3; ++a) {
            r.ne[a] = g.nl[a] + 1;
            r.e0[a] = std::max(g.L0 + 8 * (g.l0[a] - 1), g.lo - 1);
            r.e1[a] = std::min(g.L0 + 8 * (g.l0[a] + g.nl[a]), g.hi + 1);
        }
        if ((rc = render_scratch(o, g.leaves(), (r.ext_leaves() + 31) / 32))) return rc;
    }
    const size_t px = (size_t)cam->width * cam->height;
    const size_t bytes = rdef::record_bytes(px, what);
    if ((rc = snap_reserve(q, bytes, 4096))) return rc;
    o->m[k].width = cam->width, o->m[k].height = cam->height, o->m[k].what = what;
    HIPCHK(hipMemsetAsync(q.dev, 0, 16, s->st));
    launch_render(s->st, r, *cam, shade ? *shade : rdef::default_shade(), f.tv, f.flags, o->neg, o->occ, (unsigned*)q.dev,
                  (what & FLUID_RENDER_RGB) ? (unsigned char*)(q.dev + rdef::rgb_at()) : nullptr,
                  (what & FLUID_RENDER_DEPTH) ? (float*)(q.dev + rdef::depth_at(px, what)) : nullptr,
                  (what & FLUID_RENDER_NORMALS) ? (float*)(q.dev + rdef::normals_at(px, what)) : nullptr);
    HIPCHK(hipGetLastError());
    if ((rc = snap_commit(o->ring, s->st, bytes))) return rc;
    o->last_px = (long)px;
    o->last_what = what;
    return FLUID_OK;
}

int fluid_render_wait(fluid_sim_t* s, fluid_image_t* out)
{
    if (int rc = snap_guard(s, RENDER_SINGLE)) return rc;
    if (!out) return fail(FLUID_ERR_ARG, "null argument");
    RenderState* o = s->render;
    int k = -1, rc = o ? snap_next_wait(o->ring, &k) : FLUID_OK;
    if (rc) return rc;
    if (k < 0) return fail(FLUID_ERR_STATE, "no render snapshot is outstanding");
    const char* host = o->ring.s[k].host;
    const RenderMeta& m = o->m[k];
    const size_t px = (size_t)m.width * m.height;
    out->width = m.width, out->height = m.height;
    out->n_hit = (int64_t) * (const uint32_t*)host;
    out->rgb = (m.what & FLUID_RENDER_RGB) ? (const uint8_t*)(host + rdef::rgb_at()) : nullptr;
    out->depth = (m.what & FLUID_RENDER_DEPTH) ? (const float*)(host + rdef::depth_at(px, m.what)) : nullptr;
    out->normals = (m.what & FLUID_RENDER_NORMALS) ? (const float*)(host + rdef::normals_at(px, m.what)) : nullptr;
    o->last_hits = (long)out->n_hit;
    return FLUID_OK;
}

int fluid_render_stats(fluid_sim_t* s, int64_t* pixels, int64_t* hits, int64_t* bytes_to_host)
{
    if (int rc = snap_guard(s, RENDER_SINGLE)) return rc;
    const RenderState* o = s->render;
    if (pixels) *pixels = o ? o->last_px : 0;
    if (hits) *hits = o ? o->last_hits : 0;
    if (bytes_to_host) *bytes_to_host = o && o->last_what ? (int64_t)rdef::record_bytes((size_t)o->last_px, o->last_what) : 0;
    return FLUID_OK;
}

}  // extern "C"
