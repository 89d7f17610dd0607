// `fluid` — the program `./run.sh fluid` builds and runs (reference: run.sh:1-7, main() in
// fluid.cc:1151-1514).  Host C++ only: scene set-up, the 500-step loop, the same stdout lines
// (fluid.cc:1383-1386,1456,1486,1491,1499-1502) and one density grid per step; every step is
// one fluid_step() call into libfluid_hip.so (hand-written HIP, gfx950).
//
// Like the reference it takes no arguments.  Environment overrides (all optional):
//   FLUID_N (121)  FLUID_PPC (10)  FLUID_STEPS (500)  FLUID_SEED (0)  FLUID_DEVICE (0)  FLUID_FLIP_BLEND (1)
//   FLUID_OUT (simulation)  — directory for mygrids<i>.vdb (fluid.cc:1371,1503-1510); "" disables output; FLUID_RAW=1 adds .f32 dumps.
//   FLUID_OUT_DENSE (0)  — 1: every step downloads the dense grid and writes both files from it on the main thread (the loop this
// program had before the leaf snapshots; same files, for comparison).
// Output by default: after step i fluid_output_snapshot lists the grid's non-zero 8^3 leaves on the device and starts their copy
// to pinned memory; the main thread goes on with step i + 1, waits for the copy (long over by then) and hands the leaf list to
// a writer thread that zips the listed leaves once and appends the grid to both files while step i + 2 runs.
//   FLUID_OUT_SURFACE=R,W (unset: off) — additionally simulation/surface<i>.vdb per step: the liquid surface as the narrow-band level
// set of spheres of radius R voxels around the particles, band half width W voxels (fluid_sdf_snapshot after the density snapshot,
// fluid_sdf_wait beside fluid_output_wait, fluid_write_vdb_sdf on the writer thread).  One GPU and the leaf output only: refused
// with FLUID_BLOCKS, with FLUID_OUT_DENSE=1, with an empty FLUID_OUT and with FLUID_STEPS=0.  Stdout and every other file are what they are without it.
//   FLUID_OUT_MESH=R,W (unset: off) — additionally simulation/mesh<i>.ply per step: the same surface as polygons, the surface nets of
// that level set (fluid_mesh_snapshot after the other snapshots, fluid_mesh_wait beside theirs, fluid_write_ply_mesh with voxel size
// dx on the writer thread).  With or without FLUID_OUT_SURFACE; refused where that one is.  Stdout and every other file are what
// they are without it.
//   FLUID_OUT_MESH_VEL=SCALE (unset: off; with FLUID_OUT_MESH only) — mesh<i>.ply carries vx / vy / vz per vertex, the velocity of the
// closest particles interpolated onto the vertex (include/fluid_hip.h, "liquid surface, attributes": fluid_mesh_snapshot_attr,
// fluid_mesh_wait_attr, fluid_write_ply_mesh_attr) times SCALE, a finite number.  Composes with FLUID_OUT_SMOOTH.  Refused without
// FLUID_OUT_MESH or malformed, before any handle is created.  Positions and faces are those of the file without it; unset, every file
// is byte for byte what it was.
//   FLUID_OUT_MESH_NORMALS=1, FLUID_OUT_MESH_TRIS=1 (unset or 0: off; with FLUID_OUT_MESH only) — mesh<i>.ply carries nx / ny / nz per vertex,
// the normalised gradient of the level set at the vertex, and / or its faces are two triangles per quad, cut along the shorter diagonal
// (include/fluid_hip.h, "normals and triangles": fluid_mesh_snapshot_ex, fluid_mesh_wait_ex, fluid_write_ply_mesh_ex).  Compose with
// FLUID_OUT_MESH_VEL and FLUID_OUT_SMOOTH.  Refused without FLUID_OUT_MESH or with a value other than 0 or 1, before any handle is
// created.  Unset, every file is byte for byte what it was.
// Initial particles: with the defaults (N = 121, 10 per voxel) exactly the reference's — fill(CoordBBox(-20, 20)) scattered by
// UniformPointScatter with std::mt19937(FLUID_SEED) (fluid_scene_uniform_scatter: 689210 points); any other N / PPC takes the
// scaled synthetic cube (fluid_scene_water_cube_drop).
//   FLUID_SOURCE_EVERY (0 = off) — the reference's own emitter, commented out there: at the end of step i with i % K == 0 the
// points of UniformPointScatter with std::mt19937(i+1) at 10 per voxel over fluidGrid (fluid.cc:1374-1375, 1495) are appended
// with their velocities interpolated from the grid (pos.interpFromGrid(vels, 60, containerGrid), fluid.cc:1497), i.e.
// fluid_scene_uniform_scatter(flo, fhi, 10, i+1, hi) + fluid_add_particles(..., NULL); the reference's `if (i%5 == 0)` gate
// (fluid.cc:1379) is K here.  The box is the one of the initial scene (-20..20 at N = 121, scaled with N like the cube); the
// particle count is printed after every step.
//   FLUID_BLOCKS=AxBxC (unset: one GPU, everything above) — the grid cut into A x B x C blocks (fluid_create_dist), one host thread
// of this process per block over the in-process transport (fluid_local_comm_create); block r runs on device r % FLUID_DEVICES (1).
// Cut planes by particle count (fluid_partition_blocks on the initial particles), global ids = index in the initial set.
// FLUID_DIST_SOLVE=decomposed|replicated (unset: the library's choice by N); FLUID_REBALANCE_EVERY=K (0) with FLUID_REBALANCE_RATIO
// (1.5) moves the planes as the water moves.  Output: fluid_dist_output_every(1) on every block — each step leaves the list of the
// non-zero leaves of the block it owned — the main thread waits for all blocks, releases the next step, merges the lists
// (fluid_leaf_grids_merge, two merge buffers in turn) and hands the grid to the same writer thread: the same files.  The stdout
// lines are rank 0's numbers.  FLUID_SOURCE_EVERY and FLUID_OUT_DENSE=1 are refused with FLUID_BLOCKS.
//   FLUID_BLOCKS_SURFACE=R,W (unset: off; with FLUID_BLOCKS only) — additionally simulation/surface<i>.vdb per step, the file
// FLUID_OUT_SURFACE writes on one GPU: every block thread takes fluid_dist_sdf_snapshot of its live particles after its step and
// waits for it, the main thread merges the blocks' lists (fluid_sdf_grids_merge, two merge buffers in turn) and hands the grid to
// the writer thread beside the density job.  Refused without FLUID_BLOCKS, malformed, with an empty FLUID_OUT and with
// FLUID_STEPS=0, before any handle is created.  Stdout and every other file are what they are without it.
//   FLUID_BLOCKS_MESH=R,W (unset: off; with FLUID_BLOCKS only) — additionally simulation/mesh<i>.ply per step, the file FLUID_OUT_MESH
// writes on one GPU: the blocks' level-set lists are merged as for FLUID_BLOCKS_SURFACE (with both set R,W must be the same numbers
// and one snapshot per step serves both), and the writer thread meshes the merged list (fluid_sdf_mesh) and writes it
// (fluid_write_ply_mesh, voxel size dx) beside the density job.  Refused without FLUID_BLOCKS, malformed, with other numbers than
// FLUID_BLOCKS_SURFACE, with an empty FLUID_OUT and with FLUID_STEPS=0, before any handle is created.
//   FLUID_BLOCKS_MESH_VEL=SCALE (unset: off; with FLUID_BLOCKS_MESH only) — mesh<i>.ply carries vx / vy / vz per vertex times SCALE: every
// block takes fluid_dist_sdf_snapshot_attr, the main thread merges the rank records (fluid_sdf_attr_grids_merge: include/fluid_hip.h,
// "liquid surface, attributes (decomposed runs)"), the writer thread adds fluid_sdf_mesh_attr and writes fluid_write_ply_mesh_attr.
// Refused without FLUID_BLOCKS_MESH or malformed.  Stdout and every other file are what they are without the two.
//   FLUID_BLOCKS_MESH_NORMALS=1, FLUID_BLOCKS_MESH_TRIS=1 (unset or 0: off; with FLUID_BLOCKS_MESH only) — the same two options for the block
// run's mesh<i>.ply, through the host functions on the writer thread (fluid_sdf_mesh_normals on the merged list, after the filter if
// FLUID_OUT_SMOOTH is set; fluid_mesh_triangles on the mesh).  Refused without FLUID_BLOCKS_MESH or with a value other than 0 or 1.
//   FLUID_OUT_RENDER=R,W[,WIDTHxHEIGHT] (unset: off; default 640x360) — additionally simulation/frame<i>.png per step: the level set of
// the same R,W ray-cast on the device (include/fluid_hip.h, "liquid surface as an image": fluid_render_snapshot beside the other
// snapshots, fluid_write_png on the writer thread), white on black, seen by fluid_camera_look_at from FLUID_OUT_RENDER_EYE=x,y,z
// (index space; default a three-quarter view from outside the grid, N * (-0.9, 0.5, -1.2)) towards the origin, up = +y, 40 degrees,
// step 0.5.  Composes with FLUID_OUT_SMOOTH.  One GPU and the leaf output only, refused where FLUID_OUT_SURFACE is.
//   FLUID_BLOCKS_RENDER=R,W[,WIDTHxHEIGHT] (unset: off; with FLUID_BLOCKS only) — the same file from a block run: the writer thread
// renders the merged list (fluid_sdf_render, after the filter if FLUID_OUT_SMOOTH is set).  The same R,W as FLUID_BLOCKS_SURFACE /
// FLUID_BLOCKS_MESH when set together.  Without these variables stdout and every file are what they are.
//   FLUID_OUT_SMOOTH=W,K[,OFFSET] (unset: off) — what FLUID_OUT_SURFACE, FLUID_OUT_MESH, FLUID_BLOCKS_SURFACE and FLUID_BLOCKS_MESH write is the level set
// after K box filters of width W voxels and the offset (include/fluid_hip.h, "liquid surface, smoothed"): on one GPU the snapshots
// are fluid_sdf_snapshot_filtered / fluid_mesh_snapshot_filtered; a block run filters the merged list on the main thread
// (fluid_sdf_filter, two buffers in turn) before it goes to the writer thread.  Refused malformed, outside the filter's limits, or
// with none of the four set, before any handle is created.  Without it stdout and every file are what they were.
//   FLUID_OUT_SMOOTH_KIND=box|median|laplacian|curvature (unset: box; with FLUID_OUT_SMOOTH only) — the filter FLUID_OUT_SMOOTH runs K
// iterations of (include/fluid_hip.h, "liquid surface, flows"), for everything FLUID_OUT_SMOOTH applies to: a median takes W = 1 or 2,
// laplacian and curvature W = 1.  One GPU through fluid_sdf_set_filter_kind, a block run through fluid_sdf_flow on the main thread
// after the merge, tracked and grown as FLUID_OUT_TRACK says.  Refused with another name, without FLUID_OUT_SMOOTH or with a W the
// kind does not admit, before any handle is created.
//   FLUID_OUT_TRACK=N[,TRIM] (unset: off; with FLUID_OUT_SMOOTH only; TRIM defaults to 1) — the filter runs tracked: N normalisation
// passes (0..8) and, with TRIM = 1, the trim after every box iteration and every offset step (include/fluid_hip.h, "liquid
// surface, renormalised"), for everything FLUID_OUT_SMOOTH applies to: one GPU through fluid_sdf_set_track, a block run through
// fluid_sdf_filter_tracked on the main thread after the merge (the trim can shorten the list).  Refused without FLUID_OUT_SMOOTH,
// malformed or outside the limits, or with FLUID_BLOCKS_MESH_VEL (the block driver does not gather attributes through `kept`),
// before any handle is created.  Without it stdout and every file are what they were.
//   FLUID_OUT_TRACK=N,1,GROW (GROW 0 or 1, default 0) — with GROW = 1 every track begins with a dilation of the band (include/fluid_hip.h,
// "liquid surface, grown band"; N >= 1 and TRIM = 1 are required, and |OFFSET| of FLUID_OUT_SMOOTH may reach 4 voxels): one GPU
// through fluid_sdf_set_track_grow, a block run through fluid_sdf_filter_grown after the merge, which returns the attributes in
// full — so FLUID_BLOCKS_MESH_VEL is accepted with GROW = 1.
//   FLUID_OUT_TRACK_SCHEME=first|hjweno5 (default first; with FLUID_OUT_TRACK only) — the spatial scheme of the normalisation passes:
// first-order upwind, or HJWENO5, the library's own default (include/fluid_hip.h, "liquid surface, renormalised: HJWENO5").  One GPU
// through fluid_sdf_set_track, a block run through the scheme field of the track its host function is given.  Refused with another
// word or without FLUID_OUT_TRACK, before any handle is created.
//   FLUID_OUT_SURFACE_KIND=spheres|averaged[,H] (unset: spheres; H defaults to 3) — the level set FLUID_OUT_SURFACE, FLUID_OUT_MESH and
// FLUID_OUT_RENDER take from the particles: the union of spheres, or the distance to the weighted average of the particle positions
// within H voxels, 0 < H <= 4 (include/fluid_hip.h, "liquid surface, averaged positions"), through fluid_sdf_set_surface; the
// filters of FLUID_OUT_SMOOTH follow it as they follow the spheres.  One GPU only.  Refused with another word, an H outside the
// limits, none of the three set, with FLUID_BLOCKS (a block run takes FLUID_BLOCKS_SURFACE_KIND) or with
// FLUID_OUT_MESH_VEL (an average of positions has no closest particle), before any handle is created.
//   FLUID_BLOCKS_SURFACE_KIND=spheres|averaged[,H] (unset: spheres; H defaults to 3; read with FLUID_BLOCKS only) — the same choice for
// what FLUID_BLOCKS_SURFACE, FLUID_BLOCKS_MESH and FLUID_BLOCKS_RENDER take: with averaged every block thread takes the rank record
// of its live particles (fluid_dist_sdf_snapshot_avg: minimum and weighted integer sums per voxel) and the main thread merges the
// records (fluid_sdf_avg_grids_merge; include/fluid_hip.h, "liquid surface, averaged positions (decomposed runs)"): the merged list
// is byte for byte the one-GPU list, and everything after the merge — FLUID_OUT_SMOOTH*, mesh, normals, triangles, image, file —
// goes on as after fluid_sdf_grids_merge.  Refused with another word, an H outside the limits, none of the three set, or with
// FLUID_BLOCKS_MESH_VEL (an average of positions has no closest particle), before any handle is created.
//   FLUID_OUT_SURFACE_TRAILS=SHUTTER[,DELTA[,RMIN[,MAX]]] (unset: off) — the level set FLUID_OUT_SURFACE, FLUID_OUT_MESH and
// FLUID_OUT_RENDER take from the particles is that of their velocity trails (include/fluid_hip.h, "liquid surface, velocity trails"),
// through fluid_sdf_set_trails: SHUTTER is the time a trail covers, a finite number >= 0 or the word dt, the dt FLIPadvect wrote in
// the step the snapshot follows (fluid_step_stats_t.dt_out; the setting is renewed every step); DELTA > 0 the spacing factor
// (default 1); RMIN > 0 the radius at the trail's end in voxels (default: half the smallest R of the three outputs), at most every
// such R; MAX in 1..32 the most instances of a particle (default 16).  One GPU only.  Refused outside these limits, with none of
// the three set, with FLUID_OUT_SURFACE_KIND=averaged, FLUID_OUT_MESH_VEL (trails carry no attributes) or FLUID_BLOCKS (a block run
// takes FLUID_BLOCKS_SURFACE_TRAILS), before any handle is created.
//   FLUID_BLOCKS_SURFACE_TRAILS=SHUTTER[,DELTA[,RMIN[,MAX]]] (unset: off; read with FLUID_BLOCKS only) — the same choice, with the same
// grammar, defaults and word dt, for what FLUID_BLOCKS_SURFACE, FLUID_BLOCKS_MESH[_NORMALS|_TRIS] and FLUID_BLOCKS_RENDER take: every
// block thread takes the rank record of its live particles' instances (fluid_dist_sdf_snapshot_trails, the trails an argument; with
// dt the shutter is the block's own dt_out of the step just taken, the same double on every block) in the place of
// fluid_dist_sdf_snapshot, and the main thread merges the plain lists as before (fluid_sdf_grids_merge; include/fluid_hip.h, "liquid
// surface, velocity trails (decomposed runs)"): the merged list is byte for byte the one-GPU list of all particles, and
// FLUID_OUT_SMOOTH*, FLUID_OUT_TRACK*, mesh, image and file go on unchanged.  Refused malformed, with RMIN > R, with none of the three
// set, with FLUID_BLOCKS_SURFACE_KIND=averaged or with FLUID_BLOCKS_MESH_VEL (trails carry no attributes), before any handle is created.
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sys/stat.h>

#include "fluid_hip.h"

static long env_long(const char* k, long d)
{
    const char* v = getenv(k);
    return v && *v ? atol(v) : d;
}

// FLUID_RAW=1: the bare float32 dump (int32 n, then n^3 floats, z fastest)
// a 0 / 1 switch that adds to what `base` writes: 0 = off (unset, empty or "0"), 1 = on, -1 = refused (the message is printed)
static int env_option(const char* name, const char* base, bool base_set, const char* adds)
{
    const char* v = getenv(name);
    if (!v || !*v) return 0;
    const std::string t = v;
    if (t != "0" && t != "1") {
        std::cerr << name << " must be 0 or 1 (it adds " << adds << " to what " << base << " writes)" << std::endl;
        return -1;
    }
    if (!base_set) {
        std::cerr << name << " adds " << adds << " to what " << base << "=R,W writes: it is not set" << std::endl;
        return -1;
    }
    return t == "1";
}

// "SHUTTER[,DELTA[,RMIN[,MAX]]]" of FLUID_OUT_SURFACE_TRAILS / FLUID_BLOCKS_SURFACE_TRAILS into *t; *dt: SHUTTER is the word dt.  Rsmall: the
// smallest (float) R of the outputs that are set, +inf if none is (RMIN defaults to half of it).  false: malformed or outside the
// limits, and the usage is printed under the variable's name
static bool parse_trails(const char* name, const char* value, double Rsmall, fluid_sdf_trails_t* t, bool* dt)
{
    const std::string v = value;
    std::vector<std::string> part;
    for (size_t at = 0;;) {
        const size_t comma = v.find(',', at);
        part.push_back(v.substr(at, comma == std::string::npos ? comma : comma - at));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    *t = fluid_sdf_trails_t{0.0, 1.0, 0.0, 16, 0};
    *dt = false;
    t->radius_min = std::isfinite(Rsmall) ? 0.5 * Rsmall : 0.5;
    char tail = 0;
    long maxi = 16;
    bool ok = part.size() >= 1 && part.size() <= 4;
    if (ok && part[0] == "dt") *dt = true;
    else ok = ok && sscanf(part[0].c_str(), "%lf%c", &t->shutter, &tail) == 1;
    ok = ok && (part.size() < 2 || sscanf(part[1].c_str(), "%lf%c", &t->delta, &tail) == 1);
    ok = ok && (part.size() < 3 || sscanf(part[2].c_str(), "%lf%c", &t->radius_min, &tail) == 1);
    ok = ok && (part.size() < 4 || sscanf(part[3].c_str(), "%ld%c", &maxi, &tail) == 1);
    ok = ok && maxi >= 1 && maxi <= 32;
    t->max_instances = (int32_t)(ok ? maxi : 16);
    if (!ok || !(t->shutter >= 0) || !std::isfinite(t->shutter) || !(t->delta > 0) || !std::isfinite(t->delta) || !(t->radius_min > 0) ||
        !std::isfinite(t->radius_min)) {
        std::cerr << name << " must be SHUTTER[,DELTA[,RMIN[,MAX]]]: SHUTTER a finite time >= 0 or the word dt, DELTA > 0, RMIN > 0 (voxels), MAX in 1..32, e.g. dt,1,0.5,16" << std::endl;
        return false;
    }
    return true;
}

// "R,W[,WIDTHxHEIGHT]" of FLUID_OUT_RENDER / FLUID_BLOCKS_RENDER
static bool parse_render(const char* v, fluid_sdf_params_t* p, int* w, int* h)
{
    char tail = 0;
    *w = 640, *h = 360;
    const int got = sscanf(v, "%lf,%lf,%dx%d%c", &p->radius, &p->half_width, w, h, &tail);
    if (got == 2) {   // "R,W" alone: nothing may follow W
        int used = 0;
        return sscanf(v, "%lf,%lf%n", &p->radius, &p->half_width, &used) == 2 && v[used] == 0;
    }
    return got == 4 && *w >= 1 && *w <= 8192 && *h >= 1 && *h <= 8192 && (long)*w * *h <= (1L << 24);
}

// the camera of FLUID_OUT_RENDER / FLUID_BLOCKS_RENDER; false: FLUID_OUT_RENDER_EYE is malformed or the view is degenerate
static bool render_camera(int n, int w, int h, fluid_camera_t* cam)
{
    double eye[3] = {-0.9 * n, 0.5 * n, -1.2 * n};
    if (const char* e = getenv("FLUID_OUT_RENDER_EYE"); e && *e) {
        char tail = 0;
        if (sscanf(e, "%lf,%lf,%lf%c", &eye[0], &eye[1], &eye[2], &tail) != 3) return false;
    }
    const double target[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};
    return fluid_camera_look_at(n, eye, target, up, 40.0, w, h, 0.5, cam) == FLUID_OK;
}

static bool write_f32(const std::string& fr, int32_t n32, const float* v, size_t ncell)
{
    FILE* f = fopen(fr.c_str(), "wb");
    if (!f) return false;
    bool ok = fwrite(&n32, sizeof(n32), 1, f) == 1 && fwrite(v, sizeof(float), ncell, f) == ncell;
    return fclose(f) == 0 && ok;
}

// The writer thread: one grid at a time, in step order.  It reads the leaf list's pointers only (valid until the second following
// snapshot: the main thread waits for grid i - 2 to be written before it takes snapshot i), never the handle.
struct LeafWriter {
    std::string outdir, fin;
    fluid_vdb_writer_t* all = nullptr;
    bool raw_f32 = false;
    std::mutex m;
    std::condition_variable cv;
    fluid_leaf_grid_t job{};
    fluid_sdf_grid_t sjob{};  // FLUID_OUT_SURFACE: the same step's surface
    bool has_sjob = false;
    fluid_mesh_t mjob{};      // FLUID_OUT_MESH: the same step's mesh
    bool has_mjob = false;
    fluid_mesh_attr_t majob{};   // FLUID_OUT_MESH_VEL: its vertex velocities
    bool has_majob = false;
    fluid_mesh_ex_t mxjob{};     // FLUID_OUT_MESH_NORMALS / _TRIS: its normals and triangles (and velocities)
    unsigned mesh_what = 0;      // FLUID_MESH_* bits of what mesh<i>.ply carries, one GPU or blocks
    float vel_scale = 1.0f;
    float voxel = 1.0f;
    fluid_sdf_grid_t bjob{};     // FLUID_BLOCKS_MESH: the merged level set this thread meshes
    bool has_bjob = false;
    fluid_sdf_attr_t bajob{};    // FLUID_BLOCKS_MESH_VEL: its merged attributes
    bool has_bajob = false;
    bool b_mesh = false, b_render = false;   // what this thread makes of bjob: mesh<i>.ply (FLUID_BLOCKS_MESH), frame<i>.png (FLUID_BLOCKS_RENDER)
    fluid_camera_t cam{};        // FLUID_BLOCKS_RENDER: the camera
    fluid_image_t ijob{};        // FLUID_OUT_RENDER: the same step's image
    bool has_ijob = false;
    int job_step = -1;        // step whose grid is waiting (-1: none)
    int done = 0;             // grids written
    bool quit = false;
    std::string error;        // first failure: the file that could not be written
    std::thread th;
    void start() { th = std::thread([this] { run(); }); }
    ~LeafWriter() { stop(); }   // (an early return of main: the grid in hand is still written)
    // FLUID_BLOCKS_MESH: the surface nets of the merged list, with vertex velocities when `at` is given, into `fm`
    // fluid_write_ply_mesh_ex of the parts mesh_what names; a part an empty mesh lacks still gets its header lines
    bool write_ex(const std::string& fm, const fluid_mesh_t& mg, fluid_mesh_ex_t ex) const
    {
        static const float none_f[3] = {0.0f, 0.0f, 0.0f};
        static const uint32_t none_u[3] = {0, 0, 0};
        if ((mesh_what & FLUID_MESH_VELOCITY) && !ex.velocity) ex.velocity = none_f;
        if ((mesh_what & FLUID_MESH_NORMALS) && !ex.normals) ex.normals = none_f;
        if ((mesh_what & FLUID_MESH_TRIANGLES) && !ex.triangles) ex.triangles = none_u, ex.n_triangles = 2 * mg.n_quads;
        return fluid_write_ply_mesh_ex(fm.c_str(), &mg, &ex, voxel, vel_scale) == FLUID_OK;
    }
    bool mesh_blocks(const std::string& fm, const fluid_sdf_grid_t& g, const fluid_sdf_attr_t* at, std::vector<float>& v, std::vector<uint32_t>& q,
                     std::vector<float>& w, std::vector<float>& nr, std::vector<uint32_t>& tr)
    {
        int64_t nq = 0;
        const int64_t nv = fluid_sdf_mesh(&g, 0, 0, nullptr, nullptr, &nq);
        if (nv < 0) return false;
        v.resize(3 * (size_t)nv + 3), q.resize(4 * (size_t)nq + 4);
        if (nv && fluid_sdf_mesh(&g, nv, nq, v.data(), q.data(), &nq) != nv) return false;
        const fluid_mesh_t mg{g.n, nv, nq, g.radius, g.half_width, g.background, nv ? v.data() : nullptr, nq ? q.data() : nullptr};
        if (mesh_what & (FLUID_MESH_NORMALS | FLUID_MESH_TRIANGLES)) {
            fluid_mesh_ex_t ex{};
            if (at) {
                w.resize(3 * (size_t)nv + 3);
                if (nv && fluid_sdf_mesh_attr(&g, at, nv, w.data()) != nv) return false;
                ex.velocity = nv ? w.data() : nullptr;
            }
            if (mesh_what & FLUID_MESH_NORMALS) {
                nr.resize(3 * (size_t)nv + 3);
                if (nv && fluid_sdf_mesh_normals(&g, nv, nr.data()) != nv) return false;
                ex.normals = nv ? nr.data() : nullptr;
            }
            if (mesh_what & FLUID_MESH_TRIANGLES) {
                tr.resize(6 * (size_t)nq + 6);
                if (nq && fluid_mesh_triangles(&mg, 2 * nq, tr.data()) != 2 * nq) return false;
                ex.triangles = nq ? tr.data() : nullptr;
                ex.n_triangles = nq ? 2 * nq : 0;
            }
            return write_ex(fm, mg, ex);
        }
        if (!at) return fluid_write_ply_mesh(fm.c_str(), &mg, voxel) == FLUID_OK;
        w.resize(3 * (size_t)nv + 3);
        if (nv && fluid_sdf_mesh_attr(&g, at, nv, w.data()) != nv) return false;
        const fluid_mesh_attr_t ma{nv, nv ? w.data() : nullptr};
        return fluid_write_ply_mesh_attr(fm.c_str(), &mg, &ma, voxel, vel_scale) == FLUID_OK;
    }
    void run()
    {
        std::vector<float> dense, bv, bw, bn;
        std::vector<uint32_t> bq, bt;
        std::vector<uint8_t> pix;
        for (;;) {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return job_step >= 0 || quit; });
            if (job_step < 0) return;
            const fluid_leaf_grid_t g = job;
            const fluid_sdf_grid_t sg = sjob;
            const bool has_sg = has_sjob;
            const fluid_mesh_t mg = mjob;
            const bool has_mg = has_mjob;
            const fluid_mesh_attr_t ma = majob;
            const bool has_ma = has_majob;
            const fluid_mesh_ex_t mx = mxjob;
            const fluid_sdf_grid_t bg = bjob;
            const bool has_bg = has_bjob;
            const fluid_sdf_attr_t ba = bajob;
            const bool has_ba = has_bajob;
            const fluid_image_t im = ijob;
            const bool has_im = has_ijob;
            const int i = job_step;
            lk.unlock();
            std::string bad;
            // file2.write(grids2) of fluid.cc:1503-1504 and this step's grid of file.write(grids), :1508: zipped once, written twice
            const std::string fn = outdir + "/mygrids" + std::to_string(i) + ".vdb";
            fluid_vdb_writer_t* ws[2] = {nullptr, all};
            if (fluid_vdb_open(fn.c_str(), g.n, 1, FLUID_VDB_ZIP_ACTIVE_MASK, &ws[0]) != FLUID_OK) bad = fn;
            else {
                if (fluid_vdb_append_leaves(ws, 2, &g) != FLUID_OK) bad = fn + " / " + fin;
                if (fluid_vdb_close(ws[0]) != FLUID_OK && bad.empty()) bad = fn;
            }
            if (has_sg && bad.empty()) {
                const std::string fs = outdir + "/surface" + std::to_string(i) + ".vdb";
                if (fluid_write_vdb_sdf(fs.c_str(), &sg, FLUID_VDB_ZIP_ACTIVE_MASK) != FLUID_OK) bad = fs;
            }
            if (has_mg && bad.empty()) {
                const std::string fm = outdir + "/mesh" + std::to_string(i) + ".ply";
                if (mesh_what & (FLUID_MESH_NORMALS | FLUID_MESH_TRIANGLES)) {
                    if (!write_ex(fm, mg, mx)) bad = fm;
                } else if ((has_ma ? fluid_write_ply_mesh_attr(fm.c_str(), &mg, &ma, voxel, vel_scale) : fluid_write_ply_mesh(fm.c_str(), &mg, voxel)) != FLUID_OK) bad = fm;
            }
            if (has_bg && b_mesh && bad.empty()) {
                const std::string fm = outdir + "/mesh" + std::to_string(i) + ".ply";
                if (!mesh_blocks(fm, bg, has_ba ? &ba : nullptr, bv, bq, bw, bn, bt)) bad = fm;
            }
            if (has_im && bad.empty()) {
                const std::string fp = outdir + "/frame" + std::to_string(i) + ".png";
                if (!im.rgb || fluid_write_png(fp.c_str(), im.width, im.height, im.rgb) != FLUID_OK) bad = fp;
            }
            if (has_bg && b_render && bad.empty()) {
                const std::string fp = outdir + "/frame" + std::to_string(i) + ".png";
                pix.resize(3 * (size_t)cam.width * cam.height);
                if (fluid_sdf_render(&bg, &cam, nullptr, FLUID_RENDER_RGB, pix.data(), nullptr, nullptr, nullptr) != FLUID_OK ||
                    fluid_write_png(fp.c_str(), cam.width, cam.height, pix.data()) != FLUID_OK) bad = fp;
            }
            if (raw_f32 && bad.empty()) {
                const size_t ncell = (size_t)g.n * g.n * g.n;
                dense.resize(ncell);
                const std::string fr = outdir + "/mygrids" + std::to_string(i) + ".f32";
                if (fluid_leaves_to_dense(&g, dense.data()) != FLUID_OK || !write_f32(fr, g.n, dense.data(), ncell)) bad = fr;
            }
            lk.lock();
            if (!bad.empty() && error.empty()) error = bad;
            job_step = -1;
            done = i + 1;
            cv.notify_all();
        }
    }
    // blocks until grids 0 .. n - 1 are written; false after a failure
    bool wait_done(int n)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return done >= n; });
        return error.empty();
    }
    void submit(int step, const fluid_leaf_grid_t& g, const fluid_sdf_grid_t* surface = nullptr, const fluid_mesh_t* mesh = nullptr,
                const fluid_mesh_attr_t* mesh_attr = nullptr, const fluid_sdf_grid_t* to_mesh = nullptr, const fluid_sdf_attr_t* to_mesh_attr = nullptr,
                const fluid_mesh_ex_t* mesh_ex = nullptr, const fluid_image_t* image = nullptr)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return job_step < 0; });
        job = g;
        has_sjob = surface != nullptr;
        if (surface) sjob = *surface;
        has_mjob = mesh != nullptr;
        if (mesh) mjob = *mesh;
        has_majob = mesh && mesh_attr;
        if (has_majob) majob = *mesh_attr;
        mxjob = mesh && mesh_ex ? *mesh_ex : fluid_mesh_ex_t{};
        has_bjob = to_mesh != nullptr;
        if (to_mesh) bjob = *to_mesh;
        has_bajob = to_mesh && to_mesh_attr;
        if (has_bajob) bajob = *to_mesh_attr;
        has_ijob = image != nullptr;
        if (image) ijob = *image;
        job_step = step;
        cv.notify_all();
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            quit = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};

// ---- FLUID_BLOCKS ----------------------------------------------------------------------------------------------------------------
struct BlockCfg {
    fluid_params_t prm;
    int dims[3] = {1, 1, 1};
    int devices = 1, steps = 0, rb_every = 0;
    double rb_ratio = 1.5;
    std::string outdir;
    bool raw_f32 = false;
    bool surface = false;     // FLUID_BLOCKS_SURFACE
    fluid_sdf_params_t sp{};
    bool smooth = false;      // FLUID_OUT_SMOOTH
    fluid_sdf_filter_t sf{};
    int32_t kind = FLUID_SDF_FILTER_BOX;   // FLUID_OUT_SMOOTH_KIND
    bool track = false;       // FLUID_OUT_TRACK
    bool grow = false;        // ... with GROW = 1
    fluid_sdf_track_t tk{};
    bool mesh = false;        // FLUID_BLOCKS_MESH (its R,W are in sp: the same numbers as FLUID_BLOCKS_SURFACE's when both are set)
    bool mesh_vel = false;    // FLUID_BLOCKS_MESH_VEL
    unsigned mesh_more = 0;   // FLUID_BLOCKS_MESH_NORMALS / _TRIS: FLUID_MESH_NORMALS | FLUID_MESH_TRIANGLES
    double mesh_vel_scale = 1.0;
    bool render = false;      // FLUID_BLOCKS_RENDER (its R,W are in sp as well)
    fluid_camera_t cam{};
    bool averaged = false;    // FLUID_BLOCKS_SURFACE_KIND=averaged: the blocks take rank records of the averaged surface
    fluid_sdf_surface_t surf{FLUID_SDF_SURFACE_SPHERES, 0, 0.0};
    bool trails = false;      // FLUID_BLOCKS_SURFACE_TRAILS: the blocks take rank records of their instances
    bool trails_dt = false;   // ... with SHUTTER = dt: every block's own dt_out of the step just taken
    fluid_sdf_trails_t trl{0.0, 1.0, 0.0, 16, 0};
};

// What the main thread and the block threads share: `go` = steps released so far, done[i & 1] = blocks that finished step i.
struct BlockSync {
    std::mutex m;
    std::condition_variable cv;
    int go = 0, ready = 0, done[2] = {0, 0};
    bool failed = false;
    std::string error;
    void* group = nullptr;
    // the first failure is kept; every waiter — here and inside the transport — is woken
    void fail(const std::string& what)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            if (!failed) error = what;
            failed = true;
        }
        fluid_local_group_abort(group);
        cv.notify_all();
    }
};

static int run_blocks(const BlockCfg& cfg, const std::vector<double>& pos, int64_t np, const std::chrono::steady_clock::time_point t0)
{
    const int R = cfg.dims[0] * cfg.dims[1] * cfg.dims[2], n = cfg.prm.n, steps = cfg.steps;
    std::vector<int32_t> cuts[3];
    for (int a = 0; a < 3; ++a) cuts[a].assign(cfg.dims[a] + 1, 0);
    const int32_t dims32[3] = {cfg.dims[0], cfg.dims[1], cfg.dims[2]};
    if (fluid_partition_blocks(n, np, pos.data(), dims32, cuts[0].data(), cuts[1].data(), cuts[2].data()) != FLUID_OK) {
        std::cerr << "fluid_partition_blocks: " << fluid_last_error() << std::endl;
        return 1;
    }
    // the particles of every block: base cell round(p) (half away from zero, fluid.cc:267), clamped to the grid like the library's owner rule
    std::vector<std::vector<double>> bpos(R);
    std::vector<std::vector<uint32_t>> bids(R);
    const int lo = -(n / 2);
    for (int64_t i = 0; i < np; ++i) {
        int b[3];
        for (int a = 0; a < 3; ++a) {
            long c = std::lround(pos[3 * i + a]) - lo;
            c = c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
            int k = 0;
            while (k + 1 < cfg.dims[a] && c >= cuts[a][k + 1]) ++k;
            b[a] = k;
        }
        const int r = (b[0] * cfg.dims[1] + b[1]) * cfg.dims[2] + b[2];
        bpos[r].insert(bpos[r].end(), &pos[3 * i], &pos[3 * i] + 3);
        bids[r].push_back((uint32_t)i);
    }
    BlockSync sy;
    if (fluid_local_group_create(R, &sy.group) != FLUID_OK) {
        std::cerr << "fluid_local_group_create: " << fluid_last_error() << std::endl;
        return 1;
    }
    const bool output = !cfg.outdir.empty() && steps > 0;
    std::vector<fluid_leaf_grid_t> part[2] = {std::vector<fluid_leaf_grid_t>(R), std::vector<fluid_leaf_grid_t>(R)};
    const bool surface = output && cfg.surface, mesh = output && cfg.mesh, attr = mesh && cfg.mesh_vel;
    const bool render = output && cfg.render;
    const bool level = surface || mesh || render;   // one level-set snapshot per block and step serves all of them
    std::vector<fluid_sdf_grid_t> spart[2] = {std::vector<fluid_sdf_grid_t>(R), std::vector<fluid_sdf_grid_t>(R)};
    std::vector<fluid_sdf_attr_part_t> apart[2] = {std::vector<fluid_sdf_attr_part_t>(R), std::vector<fluid_sdf_attr_part_t>(R)};
    const bool avg = level && cfg.averaged;         // ... of the averaged surface: rank records of the minimum and the sums
    std::vector<fluid_sdf_avg_part_t> vpart[2] = {std::vector<fluid_sdf_avg_part_t>(R), std::vector<fluid_sdf_avg_part_t>(R)};
    const bool trails = level && cfg.trails;        // ... of the velocity trails: plain lists of every block's instances
    std::vector<fluid_step_stats_t> st0(2);   // rank 0's stats of step i in st0[i & 1]
    auto block = [&](int r) {
        fluid_sim_t* sim = nullptr;
        auto err = [&](const char* what) { sy.fail(std::string("block ") + std::to_string(r) + ": " + what + ": " + fluid_last_error()); };
        fluid_comm_t comm;
        fluid_params_t prm = cfg.prm;
        prm.device = cfg.prm.device + r % cfg.devices;
        fluid_decomp_t dc;
        for (int a = 0; a < 3; ++a) { dc.dims[a] = cfg.dims[a]; dc.cuts[a] = cuts[a].data(); }
        bool ok = true;
        if (fluid_local_comm_create(sy.group, r, &comm) != FLUID_OK) { err("fluid_local_comm_create"); ok = false; }
        else if (fluid_create_dist(&prm, &comm, &dc, &sim) != FLUID_OK) { err("fluid_create_dist"); ok = false; }
        else if (fluid_upload_particles_ids(sim, (int64_t)bids[r].size(), bpos[r].data(), nullptr, bids[r].data()) != FLUID_OK) { err("fluid_upload_particles_ids"); ok = false; }
        else if (cfg.rb_every > 0 && fluid_dist_set_rebalance(sim, cfg.rb_every, cfg.rb_ratio) != FLUID_OK) { err("fluid_dist_set_rebalance"); ok = false; }
        else if (output && fluid_dist_output_every(sim, 1) != FLUID_OK) { err("fluid_dist_output_every"); ok = false; }
        {
            std::lock_guard<std::mutex> lk(sy.m);
            sy.ready++;
        }
        sy.cv.notify_all();
        for (int i = 0; ok && i < steps; ++i) {
            {
                std::unique_lock<std::mutex> lk(sy.m);
                sy.cv.wait(lk, [&] { return sy.go > i || sy.failed; });
                if (sy.failed) break;
            }
            fluid_step_stats_t st;
            if (fluid_step(sim, &st) != FLUID_OK) { err("fluid_step"); break; }
            // (the copy of this step's list is the only thing waited for here: the next step starts when the main thread says so)
            if (output && fluid_dist_output_wait(sim, &part[i & 1][r]) != FLUID_OK) { err("fluid_dist_output_wait"); break; }
            // the surface of this block's live particles as the step left them (exact whether or not the step moved the planes)
            if (avg && fluid_dist_sdf_snapshot_avg(sim, &cfg.sp, &cfg.surf) != FLUID_OK) { err("fluid_dist_sdf_snapshot_avg"); break; }
            if (avg && fluid_dist_sdf_wait_avg(sim, &vpart[i & 1][r]) != FLUID_OK) { err("fluid_dist_sdf_wait_avg"); break; }
            if (trails) {   // a plain record like the spheres': fluid_dist_sdf_wait below takes it
                fluid_sdf_trails_t t = cfg.trl;
                if (cfg.trails_dt) t.shutter = st.dt_out;   // the path of the step just taken (one double on every block)
                if (fluid_dist_sdf_snapshot_trails(sim, &cfg.sp, &t) != FLUID_OK) { err("fluid_dist_sdf_snapshot_trails"); break; }
            }
            if (level && !avg && !trails && (attr ? fluid_dist_sdf_snapshot_attr(sim, &cfg.sp) : fluid_dist_sdf_snapshot(sim, &cfg.sp)) != FLUID_OK) { err("fluid_dist_sdf_snapshot"); break; }
            if (level && !avg && (attr ? fluid_dist_sdf_wait_attr(sim, &spart[i & 1][r], &apart[i & 1][r]) : fluid_dist_sdf_wait(sim, &spart[i & 1][r])) != FLUID_OK) { err("fluid_dist_sdf_wait"); break; }
            {
                std::lock_guard<std::mutex> lk(sy.m);
                if (r == 0) st0[i & 1] = st;
                sy.done[i & 1]++;
            }
            sy.cv.notify_all();
        }
        // the lists handed out belong to the handle: it stays until the main thread has merged the last one
        {
            std::unique_lock<std::mutex> lk(sy.m);
            sy.cv.wait(lk, [&] { return sy.go > steps || sy.failed; });
        }
        if (sim) fluid_destroy(sim);
    };
    std::vector<std::thread> th;
    for (int r = 0; r < R; ++r) th.emplace_back(block, r);
    auto finish = [&](int code) {
        {
            std::lock_guard<std::mutex> lk(sy.m);
            sy.go = steps + 1;
        }
        sy.cv.notify_all();
        for (auto& t : th) t.join();
        fluid_local_group_destroy(sy.group);
        if (sy.failed) std::cerr << sy.error << std::endl;
        return sy.failed && code == 0 ? 1 : code;
    };
    {
        std::unique_lock<std::mutex> lk(sy.m);
        sy.cv.wait(lk, [&] { return sy.ready == R; });
    }
    if (sy.failed) return finish(1);

    if (output) mkdir(cfg.outdir.c_str(), 0755);
    fluid_vdb_writer_t* all = nullptr;
    std::string fin;
    LeafWriter lw;
    if (output) {
        const size_t slash = cfg.outdir.find_last_of('/');
        fin = (slash == std::string::npos ? std::string() : cfg.outdir.substr(0, slash + 1)) + "mygrids.vdb";
        if (fluid_vdb_open(fin.c_str(), n, steps, FLUID_VDB_ZIP_ACTIVE_MASK, &all) != FLUID_OK) {
            sy.fail("cannot write " + fin);
            return finish(1);
        }
        lw.outdir = cfg.outdir, lw.fin = fin, lw.all = all, lw.raw_f32 = cfg.raw_f32;
        lw.voxel = (float)cfg.prm.dx;
        lw.vel_scale = (float)cfg.mesh_vel_scale;
        lw.mesh_what = cfg.mesh_more | (cfg.mesh_vel ? FLUID_MESH_VELOCITY : 0u);
        lw.b_mesh = mesh, lw.b_render = render, lw.cam = cfg.cam;
        lw.start();
    }
    // the merged grid of step i lives in buffer i & 1 until the writer thread has put grid i on disk
    std::vector<int32_t> m_org[2];
    std::vector<float> m_val[2];
    std::vector<int32_t> s_org[2];
    std::vector<float> s_val[2];
    std::vector<uint64_t> s_act[2];
    std::vector<float> s_smooth[2];   // FLUID_OUT_SMOOTH: the filtered values of the merged list
    std::vector<int32_t> t_org[2];    // FLUID_OUT_TRACK: the tracked list (the trim can shorten it)
    std::vector<uint64_t> t_act[2];
    std::vector<uint32_t> t_id[2];    // ... with GROW = 1 and FLUID_BLOCKS_MESH_VEL: the grown list's attributes
    std::vector<float> t_vel[2];
    std::vector<uint32_t> s_id[2];    // FLUID_BLOCKS_MESH_VEL: the merged attributes
    std::vector<float> s_vel[2];
    double dt = cfg.prm.max_dt, simulationTime = 0;
    auto release = [&](int upto) {
        {
            std::lock_guard<std::mutex> lk(sy.m);
            sy.go = upto;
            sy.done[(upto - 1) & 1] = 0;
        }
        sy.cv.notify_all();
    };
    if (steps > 0) release(1);
    for (int i = 0; i < steps; ++i) {
        {
            std::unique_lock<std::mutex> lk(sy.m);
            sy.cv.wait(lk, [&] { return sy.done[i & 1] == R || sy.failed; });
            if (sy.failed) break;
        }
        const fluid_step_stats_t st = st0[i & 1];
        if (i + 1 < steps) release(i + 2);   // step i + 1 runs beside the merge; its lists go to the other half of `part`
        std::cout << "2" << std::endl;
        std::cout << "3" << std::endl;
        std::cout << "DT " << dt << std::endl;
        std::cout << "Before" << std::endl;
        std::cout << "After" << std::endl;
        dt = st.dt_out;
        std::cout << "DT " << dt << std::endl;
        std::cout << "Error:\t" << st.error << std::endl;
        std::cout << "Iteration:\t" << i + 1 << std::endl;
        simulationTime += dt;
        std::cout << "Time delta:\t" << simulationTime << std::endl;
        if (!output) continue;
        if (!lw.wait_done(i - 1)) { sy.fail("cannot write " + lw.error); break; }
        const int64_t k = fluid_leaf_grids_merge(part[i & 1].data(), R, 0, nullptr, nullptr);
        if (k < 0) { sy.fail("fluid_leaf_grids_merge: the blocks' leaf lists do not merge"); break; }
        auto& org = m_org[i & 1];
        auto& val = m_val[i & 1];
        if (org.size() < 3 * (size_t)k) { org.resize(3 * (size_t)k + 3 * 64); val.resize(512 * ((size_t)k + 64)); }
        if (fluid_leaf_grids_merge(part[i & 1].data(), R, k, org.data(), val.data()) != k) { sy.fail("fluid_leaf_grids_merge: the blocks' leaf lists do not merge"); break; }
        fluid_sdf_grid_t sg{};
        fluid_sdf_attr_t sat{};
        if (level) {
            const auto& sp = spart[i & 1];
            const auto& ap = apart[i & 1];
            const auto& vp = vpart[i & 1];
            const int64_t ks = avg    ? fluid_sdf_avg_grids_merge(vp.data(), R, 0, nullptr, nullptr, nullptr)
                               : attr ? fluid_sdf_attr_grids_merge(sp.data(), ap.data(), R, 0, nullptr, nullptr, nullptr, nullptr, nullptr)
                                      : fluid_sdf_grids_merge(sp.data(), R, 0, nullptr, nullptr, nullptr);
            if (ks < 0) { sy.fail(avg ? "fluid_sdf_avg_grids_merge: the blocks' rank records do not merge" : "fluid_sdf_grids_merge: the blocks' surface lists do not merge"); break; }
            auto& so = s_org[i & 1];
            auto& sv = s_val[i & 1];
            auto& sa = s_act[i & 1];
            auto& si = s_id[i & 1];
            auto& sw = s_vel[i & 1];
            if (so.size() < 3 * (size_t)ks) { so.resize(3 * ((size_t)ks + 64)); sv.resize(512 * ((size_t)ks + 64)); sa.resize(8 * ((size_t)ks + 64)); }
            if (attr && si.size() < 512 * (size_t)ks) { si.resize(512 * ((size_t)ks + 64)); sw.resize(1536 * ((size_t)ks + 64)); }
            if (ks && (avg    ? fluid_sdf_avg_grids_merge(vp.data(), R, ks, so.data(), sv.data(), sa.data())
                       : attr ? fluid_sdf_attr_grids_merge(sp.data(), ap.data(), R, ks, so.data(), sv.data(), sa.data(), si.data(), sw.data())
                              : fluid_sdf_grids_merge(sp.data(), R, ks, so.data(), sv.data(), sa.data())) != ks) { sy.fail("the blocks' surface lists do not merge: the second call disagrees with the count"); break; }
            sat = fluid_sdf_attr_t{(int32_t)ks, attr && ks ? si.data() : nullptr, attr && ks ? sw.data() : nullptr};
            sg = fluid_sdf_grid_t{n, (int32_t)ks, avg ? vp[0].background : sp[0].background, avg ? vp[0].radius : sp[0].radius,
                                  avg ? vp[0].half_width : sp[0].half_width, ks ? so.data() : nullptr, ks ? sv.data() : nullptr, ks ? sa.data() : nullptr};
            if (cfg.smooth && (cfg.kind != FLUID_SDF_FILTER_BOX || (cfg.track && cfg.grow)) && ks) {
                // a flow (FLUID_OUT_SMOOTH_KIND) in any of its three forms, or the grown box filter; the grown list can be longer than
                // the merged one: count, then fill
                const fluid_sdf_attr_t* in = attr ? &sat : nullptr;
                const bool flow = cfg.kind != FLUID_SDF_FILTER_BOX;
                const fluid_sdf_track_t* tk = cfg.track ? &cfg.tk : nullptr;
                auto filter = [&](int64_t cap, int32_t* o, float* v, uint64_t* a, uint32_t* id, float* vel) {
                    return flow ? fluid_sdf_flow(&sg, in, cfg.kind, &cfg.sf, tk, cfg.grow ? 1 : 0, cap, o, v, a, id, vel)
                                : fluid_sdf_filter_grown(&sg, in, &cfg.sf, &cfg.tk, cap, o, v, a, id, vel);
                };
                const int64_t kg = filter(0, nullptr, nullptr, nullptr, nullptr, nullptr);
                if (kg < 0) { sy.fail(flow ? "fluid_sdf_flow: the merged surface list, or the offset, was refused" : "fluid_sdf_filter_grown: the merged surface list, or an offset beyond 4 voxels, was refused"); break; }
                auto& sm = s_smooth[i & 1];
                auto& to = t_org[i & 1];
                auto& ta = t_act[i & 1];
                auto& ti = t_id[i & 1];
                auto& tv = t_vel[i & 1];
                if (to.size() < 3 * (size_t)kg) { to.resize(3 * ((size_t)kg + 64)); ta.resize(8 * ((size_t)kg + 64)); }
                if (sm.size() < 512 * (size_t)kg) sm.resize(512 * ((size_t)kg + 64));
                if (attr && ti.size() < 512 * (size_t)kg) { ti.resize(512 * ((size_t)kg + 64)); tv.resize(1536 * ((size_t)kg + 64)); }
                if (kg && filter(kg, to.data(), sm.data(), ta.data(), attr ? ti.data() : nullptr, attr ? tv.data() : nullptr) != kg) {
                    sy.fail("the level-set filter's second call disagrees with the count");
                    break;
                }
                sg = fluid_sdf_grid_t{n, (int32_t)kg, sg.background, sg.radius, sg.half_width, kg ? to.data() : nullptr, kg ? sm.data() : nullptr,
                                      kg ? ta.data() : nullptr};
                sat = fluid_sdf_attr_t{(int32_t)kg, attr && kg ? ti.data() : nullptr, attr && kg ? tv.data() : nullptr};
            } else if (cfg.smooth && cfg.track && ks) {
                auto& sm = s_smooth[i & 1];
                auto& to = t_org[i & 1];
                auto& ta = t_act[i & 1];
                if (sm.size() < sv.size()) sm.resize(sv.size());
                if (to.size() < so.size()) to.resize(so.size());
                if (ta.size() < sa.size()) ta.resize(sa.size());
                const int64_t kt = fluid_sdf_filter_tracked(&sg, &cfg.sf, &cfg.tk, ks, to.data(), sm.data(), ta.data(), nullptr);
                if (kt < 0) { sy.fail("fluid_sdf_filter_tracked: the merged surface list, or an offset beyond the background, was refused"); break; }
                sg = fluid_sdf_grid_t{n, (int32_t)kt, sg.background, sg.radius, sg.half_width, kt ? to.data() : nullptr, kt ? sm.data() : nullptr,
                                      kt ? ta.data() : nullptr};
            } else if (cfg.smooth && ks) {
                auto& sm = s_smooth[i & 1];
                if (sm.size() < sv.size()) sm.resize(sv.size());
                if (fluid_sdf_filter(&sg, &cfg.sf, sm.data()) != FLUID_OK) { sy.fail("fluid_sdf_filter: the merged surface list was refused"); break; }
                sg.values = sm.data();
            }
        }
        lw.submit(i, fluid_leaf_grid_t{n, (int32_t)k, k ? org.data() : nullptr, k ? val.data() : nullptr}, surface ? &sg : nullptr, nullptr, nullptr,
                  mesh || render ? &sg : nullptr, attr ? &sat : nullptr);
    }
    bool ok = !sy.failed;
    if (output) {
        if (ok && !lw.wait_done(steps)) { sy.fail("cannot write " + lw.error); ok = false; }
        lw.stop();
        if (all && fluid_vdb_close(all) != FLUID_OK && ok) { sy.fail("cannot write " + fin); ok = false; }
    }
    const int code = finish(ok ? 0 : 1);
    if (code) return code;
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "Time Taken " << sec / 60 << " minutes" << std::endl;
    return 0;
}

int main(int, char**)
{
    const auto t0 = std::chrono::steady_clock::now();
    fluid_params_t prm;
    fluid_default_params(&prm);
    prm.n = (int32_t)env_long("FLUID_N", 121);
    prm.device = (int32_t)env_long("FLUID_DEVICE", 0);
    const int ppc = (int)env_long("FLUID_PPC", 10);          // 10 points per voxel, fluid.cc:1349
    const int steps = (int)env_long("FLUID_STEPS", 500);     // fluid.cc:1368
    const uint64_t seed = (uint64_t)env_long("FLUID_SEED", 0);  // mt19937(0), fluid.cc:1348
    if (const char* b = getenv("FLUID_FLIP_BLEND")) prm.flip_blend = atof(b);  // default 1 = the reference's pure FLIP
    const char* outenv = getenv("FLUID_OUT");
    const std::string outdir = outenv ? outenv : "simulation";
    const bool raw_f32 = env_long("FLUID_RAW", 0) != 0;
    const long src_every = env_long("FLUID_SOURCE_EVERY", 0);
    const bool out_dense = env_long("FLUID_OUT_DENSE", 0) != 0;
    const char* blocks = getenv("FLUID_BLOCKS");
    const char* surf = getenv("FLUID_OUT_SURFACE");
    const bool surface = surf && *surf;
    fluid_sdf_params_t sp{};
    if (surface) {
        char tail = 0;
        if (sscanf(surf, "%lf,%lf%c", &sp.radius, &sp.half_width, &tail) != 2) {
            std::cerr << "FLUID_OUT_SURFACE must be R,W (sphere radius and band half width in voxels), e.g. 1.5,2.5" << std::endl;
            return 1;
        }
        if ((blocks && *blocks) || out_dense) {
            std::cerr << "FLUID_OUT_SURFACE cannot be combined with " << (out_dense ? "FLUID_OUT_DENSE=1" : "FLUID_BLOCKS (a block run takes FLUID_BLOCKS_SURFACE=R,W)") << std::endl;
            return 1;
        }
        if (outdir.empty() || steps <= 0) {
            std::cerr << "FLUID_OUT_SURFACE needs an output directory and at least one step (FLUID_OUT is empty or FLUID_STEPS is 0)" << std::endl;
            return 1;
        }
    }
    const char* menv = getenv("FLUID_OUT_MESH");
    const bool mesh = menv && *menv;
    fluid_sdf_params_t mp{};
    if (mesh) {
        char tail = 0;
        if (sscanf(menv, "%lf,%lf%c", &mp.radius, &mp.half_width, &tail) != 2) {
            std::cerr << "FLUID_OUT_MESH must be R,W (sphere radius and band half width in voxels), e.g. 1.5,2.5" << std::endl;
            return 1;
        }
        if ((blocks && *blocks) || out_dense) {
            std::cerr << "FLUID_OUT_MESH cannot be combined with " << (out_dense ? "FLUID_OUT_DENSE=1" : "FLUID_BLOCKS (a block run meshes its merged surface on the host: fluid_sdf_mesh)") << std::endl;
            return 1;
        }
        if (outdir.empty() || steps <= 0) {
            std::cerr << "FLUID_OUT_MESH needs an output directory and at least one step (FLUID_OUT is empty or FLUID_STEPS is 0)" << std::endl;
            return 1;
        }
    }
    const char* mvenv = getenv("FLUID_OUT_MESH_VEL");
    const bool mesh_vel = mvenv && *mvenv;
    double mesh_vel_scale = 1.0;
    if (mesh_vel) {
        char tail = 0;
        if (sscanf(mvenv, "%lf%c", &mesh_vel_scale, &tail) != 1 || !std::isfinite(mesh_vel_scale) || !std::isfinite((float)mesh_vel_scale)) {
            std::cerr << "FLUID_OUT_MESH_VEL must be SCALE, a finite number the vertex velocities are multiplied by, e.g. 1" << std::endl;
            return 1;
        }
        if (!mesh) {
            std::cerr << "FLUID_OUT_MESH_VEL adds velocities to what FLUID_OUT_MESH=R,W writes (one GPU): it is not set" << std::endl;
            return 1;
        }
    }
    unsigned mesh_more = 0;
    for (int k = 0; k < 2; ++k) {
        const int on = env_option(k ? "FLUID_OUT_MESH_TRIS" : "FLUID_OUT_MESH_NORMALS", "FLUID_OUT_MESH", mesh, k ? "triangles" : "vertex normals");
        if (on < 0) return 1;
        if (on) mesh_more |= k ? FLUID_MESH_TRIANGLES : FLUID_MESH_NORMALS;
    }
    const unsigned mesh_what = mesh_more | (mesh_vel ? FLUID_MESH_VELOCITY : 0u);
    BlockCfg bc;
    if (const char* bs = getenv("FLUID_BLOCKS_SURFACE"); bs && *bs) {
        char tail = 0;
        if (sscanf(bs, "%lf,%lf%c", &bc.sp.radius, &bc.sp.half_width, &tail) != 2) {
            std::cerr << "FLUID_BLOCKS_SURFACE must be R,W (sphere radius and band half width in voxels), e.g. 1.5,2.5" << std::endl;
            return 1;
        }
        if (!(blocks && *blocks)) {
            std::cerr << "FLUID_BLOCKS_SURFACE needs FLUID_BLOCKS=AxBxC (one GPU takes FLUID_OUT_SURFACE=R,W)" << std::endl;
            return 1;
        }
        if (outdir.empty() || steps <= 0) {
            std::cerr << "FLUID_BLOCKS_SURFACE needs an output directory and at least one step (FLUID_OUT is empty or FLUID_STEPS is 0)" << std::endl;
            return 1;
        }
        bc.surface = true;
    }
    if (const char* bm = getenv("FLUID_BLOCKS_MESH"); bm && *bm) {
        char tail = 0;
        fluid_sdf_params_t bmp{};
        if (sscanf(bm, "%lf,%lf%c", &bmp.radius, &bmp.half_width, &tail) != 2) {
            std::cerr << "FLUID_BLOCKS_MESH must be R,W (sphere radius and band half width in voxels), e.g. 1.5,2.5" << std::endl;
            return 1;
        }
        if (!(blocks && *blocks)) {
            std::cerr << "FLUID_BLOCKS_MESH needs FLUID_BLOCKS=AxBxC (one GPU takes FLUID_OUT_MESH=R,W)" << std::endl;
            return 1;
        }
        if (outdir.empty() || steps <= 0) {
            std::cerr << "FLUID_BLOCKS_MESH needs an output directory and at least one step (FLUID_OUT is empty or FLUID_STEPS is 0)" << std::endl;
            return 1;
        }
        if (bc.surface && (bmp.radius != bc.sp.radius || bmp.half_width != bc.sp.half_width)) {
            std::cerr << "FLUID_BLOCKS_MESH and FLUID_BLOCKS_SURFACE must be the same R,W: one level-set snapshot per step serves both" << std::endl;
            return 1;
        }
        bc.sp = bmp;
        bc.mesh = true;
    }
    if (const char* bv = getenv("FLUID_BLOCKS_MESH_VEL"); bv && *bv) {
        char tail = 0;
        if (sscanf(bv, "%lf%c", &bc.mesh_vel_scale, &tail) != 1 || !std::isfinite(bc.mesh_vel_scale) || !std::isfinite((float)bc.mesh_vel_scale)) {
            std::cerr << "FLUID_BLOCKS_MESH_VEL must be SCALE, a finite number the vertex velocities are multiplied by, e.g. 1" << std::endl;
            return 1;
        }
        if (!bc.mesh) {
            std::cerr << "FLUID_BLOCKS_MESH_VEL adds velocities to what FLUID_BLOCKS_MESH=R,W writes: it is not set" << std::endl;
            return 1;
        }
        bc.mesh_vel = true;
    }
    for (int k = 0; k < 2; ++k) {
        const int on = env_option(k ? "FLUID_BLOCKS_MESH_TRIS" : "FLUID_BLOCKS_MESH_NORMALS", "FLUID_BLOCKS_MESH", bc.mesh, k ? "triangles" : "vertex normals");
        if (on < 0) return 1;
        if (on) bc.mesh_more |= k ? FLUID_MESH_TRIANGLES : FLUID_MESH_NORMALS;
    }
    const char* renv = getenv("FLUID_OUT_RENDER");
    const bool render = renv && *renv;
    fluid_sdf_params_t rp{};
    fluid_camera_t rcam{};
    if (render) {
        int rw = 0, rh = 0;
        if (!parse_render(renv, &rp, &rw, &rh)) {
            std::cerr << "FLUID_OUT_RENDER must be R,W[,WIDTHxHEIGHT] (sphere radius and band half width in voxels; at most 8192 a side and 2^24 pixels), e.g. 1.5,2.5,640x360" << std::endl;
            return 1;
        }
        if ((blocks && *blocks) || out_dense) {
            std::cerr << "FLUID_OUT_RENDER cannot be combined with " << (out_dense ? "FLUID_OUT_DENSE=1" : "FLUID_BLOCKS (a block run takes FLUID_BLOCKS_RENDER=R,W)") << std::endl;
            return 1;
        }
        if (outdir.empty() || steps <= 0) {
            std::cerr << "FLUID_OUT_RENDER needs an output directory and at least one step (FLUID_OUT is empty or FLUID_STEPS is 0)" << std::endl;
            return 1;
        }
        if (!render_camera(prm.n, rw, rh, &rcam)) {
            std::cerr << "FLUID_OUT_RENDER_EYE must be x,y,z (index space), away from the origin and not straight above or below it" << std::endl;
            return 1;
        }
    }
    if (const char* br = getenv("FLUID_BLOCKS_RENDER"); br && *br) {
        fluid_sdf_params_t brp{};
        int rw = 0, rh = 0;
        if (!parse_render(br, &brp, &rw, &rh)) {
            std::cerr << "FLUID_BLOCKS_RENDER must be R,W[,WIDTHxHEIGHT] (sphere radius and band half width in voxels; at most 8192 a side and 2^24 pixels), e.g. 1.5,2.5,640x360" << std::endl;
            return 1;
        }
        if (!(blocks && *blocks)) {
            std::cerr << "FLUID_BLOCKS_RENDER needs FLUID_BLOCKS=AxBxC (one GPU takes FLUID_OUT_RENDER=R,W)" << std::endl;
            return 1;
        }
        if (outdir.empty() || steps <= 0) {
            std::cerr << "FLUID_BLOCKS_RENDER needs an output directory and at least one step (FLUID_OUT is empty or FLUID_STEPS is 0)" << std::endl;
            return 1;
        }
        if ((bc.surface || bc.mesh) && (brp.radius != bc.sp.radius || brp.half_width != bc.sp.half_width)) {
            std::cerr << "FLUID_BLOCKS_RENDER must be the same R,W as FLUID_BLOCKS_SURFACE / FLUID_BLOCKS_MESH: one level-set snapshot per step serves all" << std::endl;
            return 1;
        }
        if (!render_camera(prm.n, rw, rh, &bc.cam)) {
            std::cerr << "FLUID_OUT_RENDER_EYE must be x,y,z (index space), away from the origin and not straight above or below it" << std::endl;
            return 1;
        }
        bc.sp = brp;
        bc.render = true;
    }
    const char* smenv = getenv("FLUID_OUT_SMOOTH");
    const bool smooth = smenv && *smenv;
    fluid_sdf_filter_t sf{};
    if (smooth) {
        char tail = 0;
        const int got = sscanf(smenv, "%d,%d,%lf%c", &sf.width, &sf.iterations, &sf.offset, &tail);
        if (got == 2) {   // "W,K" alone: nothing may follow K
            int used = 0;
            if (sscanf(smenv, "%d,%d%n", &sf.width, &sf.iterations, &used) != 2 || smenv[used] != 0) sf.width = 0;
            sf.offset = 0;
        }
        if ((got != 2 && got != 3) || sf.width < 1 || sf.width > 4 || sf.iterations < 0 || sf.iterations > 16 || !std::isfinite(sf.offset) ||
            !std::isfinite((float)sf.offset)) {
            std::cerr << "FLUID_OUT_SMOOTH must be W,K[,OFFSET] (box width 1..4 voxels, iterations 0..16, a finite offset), e.g. 1,4,-0.5" << std::endl;
            return 1;
        }
        if (!surface && !mesh && !bc.surface && !bc.mesh && !render && !bc.render) {
            std::cerr << "FLUID_OUT_SMOOTH smooths what FLUID_OUT_SURFACE, FLUID_OUT_MESH, FLUID_OUT_RENDER, FLUID_BLOCKS_SURFACE, FLUID_BLOCKS_MESH or FLUID_BLOCKS_RENDER write: none of them is set" << std::endl;
            return 1;
        }
        bc.smooth = true, bc.sf = sf;
    }
    int32_t smooth_kind = FLUID_SDF_FILTER_BOX;
    if (const char* kenv = getenv("FLUID_OUT_SMOOTH_KIND"); kenv && *kenv) {
        const std::string v = kenv;
        if (v == "box") smooth_kind = FLUID_SDF_FILTER_BOX;
        else if (v == "median") smooth_kind = FLUID_SDF_FILTER_MEDIAN;
        else if (v == "laplacian") smooth_kind = FLUID_SDF_FILTER_LAPLACIAN;
        else if (v == "curvature") smooth_kind = FLUID_SDF_FILTER_MEAN_CURVATURE;
        else { std::cerr << "FLUID_OUT_SMOOTH_KIND must be box, median, laplacian or curvature" << std::endl; return 1; }
        if (!smooth) {
            std::cerr << "FLUID_OUT_SMOOTH_KIND chooses the filter FLUID_OUT_SMOOTH runs: FLUID_OUT_SMOOTH is not set" << std::endl;
            return 1;
        }
        if (smooth_kind == FLUID_SDF_FILTER_MEDIAN ? sf.width > 2 : smooth_kind != FLUID_SDF_FILTER_BOX && sf.width != 1) {
            std::cerr << "FLUID_OUT_SMOOTH_KIND: a median takes W = 1 or 2 in FLUID_OUT_SMOOTH, laplacian and curvature W = 1" << std::endl;
            return 1;
        }
        bc.kind = smooth_kind;
    }
    const char* tkenv = getenv("FLUID_OUT_TRACK");
    const bool track = tkenv && *tkenv;
    bool track_grow = false;
    fluid_sdf_track_t tk{0, 1, FLUID_SDF_TRACK_FIRST_BIAS};
    if (track) {
        int used = 0, grow = 0;
        const int got = sscanf(tkenv, "%d%n,%d%n,%d%n", &tk.normalize, &used, &tk.trim, &used, &grow, &used);
        if (got < 1 || tkenv[used] != 0 || tk.normalize < 0 || tk.normalize > 8 || (tk.trim != 0 && tk.trim != 1) || (grow != 0 && grow != 1)) {
            std::cerr << "FLUID_OUT_TRACK must be N[,TRIM[,GROW]] (normalisation passes 0..8, trim 0 or 1, grow 0 or 1), e.g. 3 or 3,1 or 3,1,1" << std::endl;
            return 1;
        }
        if (grow && (tk.normalize < 1 || tk.trim != 1)) {
            std::cerr << "FLUID_OUT_TRACK: GROW = 1 needs N >= 1 and TRIM = 1 (the library's track())" << std::endl;
            return 1;
        }
        track_grow = grow != 0;
        if (!smooth) {
            std::cerr << "FLUID_OUT_TRACK renormalises what FLUID_OUT_SMOOTH filters: FLUID_OUT_SMOOTH is not set" << std::endl;
            return 1;
        }
        if (bc.mesh_vel && !track_grow) {
            std::cerr << "FLUID_OUT_TRACK cannot be combined with FLUID_BLOCKS_MESH_VEL: the trim can shorten the merged list and the block driver does not gather the attributes (GROW = 1 returns them in full)" << std::endl;
            return 1;
        }
    }
    const char* scenv = getenv("FLUID_OUT_TRACK_SCHEME");
    if (scenv && *scenv) {
        const std::string word = scenv;
        if (!track) {
            std::cerr << "FLUID_OUT_TRACK_SCHEME names the scheme FLUID_OUT_TRACK runs: FLUID_OUT_TRACK is not set" << std::endl;
            return 1;
        }
        if (word != "first" && word != "hjweno5") {
            std::cerr << "FLUID_OUT_TRACK_SCHEME must be first or hjweno5" << std::endl;
            return 1;
        }
        tk.scheme = word == "hjweno5" ? FLUID_SDF_TRACK_HJWENO5 : FLUID_SDF_TRACK_FIRST_BIAS;
    }
    fluid_sdf_surface_t skind{FLUID_SDF_SURFACE_SPHERES, 0, 0.0};
    if (const char* senv = getenv("FLUID_OUT_SURFACE_KIND"); senv && *senv) {
        const std::string v = senv;
        const size_t comma = v.find(',');
        const std::string word = v.substr(0, comma);
        double H = 3.0;
        char tail = 0;
        if ((word != "spheres" && word != "averaged") || (comma != std::string::npos && (word != "averaged" || sscanf(v.c_str() + comma + 1, "%lf%c", &H, &tail) != 1)) ||
            !(H > 0) || !((float)H > 0.0f) || !((float)H <= 4.0f)) {
            std::cerr << "FLUID_OUT_SURFACE_KIND must be spheres or averaged[,H] (influence radius in voxels, 0 < H <= 4), e.g. averaged,3" << std::endl;
            return 1;
        }
        if (blocks && *blocks) {
            std::cerr << "FLUID_OUT_SURFACE_KIND cannot be combined with FLUID_BLOCKS: it is a setting of a one-GPU handle (a block run takes FLUID_BLOCKS_SURFACE_KIND: rank records of the minimum and the four sums, merged on the host)" << std::endl;
            return 1;
        }
        if (mesh_vel) {
            std::cerr << "FLUID_OUT_SURFACE_KIND cannot be combined with FLUID_OUT_MESH_VEL: an average of positions has no closest particle to take a velocity from" << std::endl;
            return 1;
        }
        if (!surface && !mesh && !render) {
            std::cerr << "FLUID_OUT_SURFACE_KIND chooses the level set FLUID_OUT_SURFACE, FLUID_OUT_MESH or FLUID_OUT_RENDER take: none of them is set" << std::endl;
            return 1;
        }
        if (word == "averaged") skind = fluid_sdf_surface_t{FLUID_SDF_SURFACE_AVERAGED, 0, H};
    }
    bool trails = false, trails_dt = false;
    fluid_sdf_trails_t trl{0.0, 1.0, 0.0, 16, 0};
    if (const char* tenv = getenv("FLUID_OUT_SURFACE_TRAILS"); tenv && *tenv) {
        double Rsmall = INFINITY;
        if (surface) Rsmall = std::fmin(Rsmall, (double)(float)sp.radius);
        if (mesh) Rsmall = std::fmin(Rsmall, (double)(float)mp.radius);
        if (render) Rsmall = std::fmin(Rsmall, (double)(float)rp.radius);
        if (!parse_trails("FLUID_OUT_SURFACE_TRAILS", tenv, Rsmall, &trl, &trails_dt)) return 1;
        if (blocks && *blocks) {
            std::cerr << "FLUID_OUT_SURFACE_TRAILS cannot be combined with FLUID_BLOCKS: it is a setting of a one-GPU handle (a block run takes FLUID_BLOCKS_SURFACE_TRAILS: the rank record of every block's instances, merged on the host)" << std::endl;
            return 1;
        }
        if (skind.kind == FLUID_SDF_SURFACE_AVERAGED) {
            std::cerr << "FLUID_OUT_SURFACE_TRAILS cannot be combined with FLUID_OUT_SURFACE_KIND=averaged: the two surfaces exclude each other" << std::endl;
            return 1;
        }
        if (mesh_vel) {
            std::cerr << "FLUID_OUT_SURFACE_TRAILS cannot be combined with FLUID_OUT_MESH_VEL: trails carry no attributes" << std::endl;
            return 1;
        }
        if (!surface && !mesh && !render) {
            std::cerr << "FLUID_OUT_SURFACE_TRAILS chooses the level set FLUID_OUT_SURFACE, FLUID_OUT_MESH or FLUID_OUT_RENDER take: none of them is set" << std::endl;
            return 1;
        }
        if (!((double)(float)trl.radius_min <= Rsmall)) {
            std::cerr << "FLUID_OUT_SURFACE_TRAILS: RMIN must not exceed the radius R of FLUID_OUT_SURFACE, FLUID_OUT_MESH and FLUID_OUT_RENDER" << std::endl;
            return 1;
        }
        trails = true;
    }
    if (const char* benv = getenv("FLUID_BLOCKS_SURFACE_KIND"); blocks && *blocks && benv && *benv) {
        const std::string v = benv;
        const size_t comma = v.find(',');
        const std::string word = v.substr(0, comma);
        double H = 3.0;
        char tail = 0;
        if ((word != "spheres" && word != "averaged") || (comma != std::string::npos && (word != "averaged" || sscanf(v.c_str() + comma + 1, "%lf%c", &H, &tail) != 1)) ||
            !(H > 0) || !((float)H > 0.0f) || !((float)H <= 4.0f)) {
            std::cerr << "FLUID_BLOCKS_SURFACE_KIND must be spheres or averaged[,H] (influence radius in voxels, 0 < H <= 4), e.g. averaged,3" << std::endl;
            return 1;
        }
        if (word == "averaged" && bc.mesh_vel) {
            std::cerr << "FLUID_BLOCKS_SURFACE_KIND=averaged cannot be combined with FLUID_BLOCKS_MESH_VEL: an average of positions has no closest particle to take a velocity from" << std::endl;
            return 1;
        }
        if (!bc.surface && !bc.mesh && !bc.render) {
            std::cerr << "FLUID_BLOCKS_SURFACE_KIND chooses the level set FLUID_BLOCKS_SURFACE, FLUID_BLOCKS_MESH or FLUID_BLOCKS_RENDER take: none of them is set" << std::endl;
            return 1;
        }
        if (word == "averaged") bc.averaged = true, bc.surf = fluid_sdf_surface_t{FLUID_SDF_SURFACE_AVERAGED, 0, H};
    }
    if (const char* tenv = getenv("FLUID_BLOCKS_SURFACE_TRAILS"); blocks && *blocks && tenv && *tenv) {
        const bool any = bc.surface || bc.mesh || bc.render;   // (their R,W are the same numbers: bc.sp)
        const double Rsmall = any ? (double)(float)bc.sp.radius : INFINITY;
        if (!parse_trails("FLUID_BLOCKS_SURFACE_TRAILS", tenv, Rsmall, &bc.trl, &bc.trails_dt)) return 1;
        if (bc.averaged) {
            std::cerr << "FLUID_BLOCKS_SURFACE_TRAILS cannot be combined with FLUID_BLOCKS_SURFACE_KIND=averaged: the two surfaces exclude each other" << std::endl;
            return 1;
        }
        if (bc.mesh_vel) {
            std::cerr << "FLUID_BLOCKS_SURFACE_TRAILS cannot be combined with FLUID_BLOCKS_MESH_VEL: trails carry no attributes" << std::endl;
            return 1;
        }
        if (!any) {
            std::cerr << "FLUID_BLOCKS_SURFACE_TRAILS chooses the level set FLUID_BLOCKS_SURFACE, FLUID_BLOCKS_MESH or FLUID_BLOCKS_RENDER take: none of them is set" << std::endl;
            return 1;
        }
        if (!((double)(float)bc.trl.radius_min <= Rsmall)) {
            std::cerr << "FLUID_BLOCKS_SURFACE_TRAILS: RMIN must not exceed the radius R of FLUID_BLOCKS_SURFACE, FLUID_BLOCKS_MESH and FLUID_BLOCKS_RENDER" << std::endl;
            return 1;
        }
        bc.trails = true;
    }
    if (track) bc.track = true, bc.tk = tk, bc.grow = track_grow;
    if (blocks && *blocks) {
        char tail = 0;
        if (sscanf(blocks, "%dx%dx%d%c", &bc.dims[0], &bc.dims[1], &bc.dims[2], &tail) != 3 || bc.dims[0] < 1 || bc.dims[1] < 1 || bc.dims[2] < 1 ||
            (long)bc.dims[0] * bc.dims[1] * bc.dims[2] > FLUID_MAX_RANKS) {
            std::cerr << "FLUID_BLOCKS must be AxBxC with at most " << FLUID_MAX_RANKS << " blocks, e.g. 2x2x2" << std::endl;
            return 1;
        }
        if (src_every > 0 || out_dense) {
            std::cerr << "FLUID_BLOCKS cannot be combined with " << (src_every > 0 ? "FLUID_SOURCE_EVERY (sources need one GPU)" : "FLUID_OUT_DENSE=1 (a block run leaves its grid as leaf lists)") << std::endl;
            return 1;
        }
        if (const char* m = getenv("FLUID_DIST_SOLVE")) {
            const std::string v = m;
            if (v == "decomposed") prm.dist_solve = FLUID_DIST_DECOMPOSED;
            else if (v == "replicated") prm.dist_solve = FLUID_DIST_REPLICATED;
            else { std::cerr << "FLUID_DIST_SOLVE must be decomposed or replicated" << std::endl; return 1; }
        }
        bc.devices = (int)env_long("FLUID_DEVICES", 1);
        if (bc.devices < 1) bc.devices = 1;
        bc.rb_every = (int)env_long("FLUID_REBALANCE_EVERY", 0);
        if (const char* r = getenv("FLUID_REBALANCE_RATIO")) bc.rb_ratio = atof(r);
        if (bc.rb_every < 0 || !(bc.rb_ratio >= 1.0)) { std::cerr << "FLUID_REBALANCE_EVERY must be >= 0 and FLUID_REBALANCE_RATIO >= 1" << std::endl; return 1; }
    }

    fluid_sim_t* sim = nullptr;
    if (!(blocks && *blocks) && fluid_create(&prm, &sim) != FLUID_OK) {
        std::cerr << "fluid_create: " << fluid_last_error() << std::endl;
        return 1;
    }
    if (sim && smooth_kind != FLUID_SDF_FILTER_BOX && fluid_sdf_set_filter_kind(sim, smooth_kind) != FLUID_OK) {
        std::cerr << "fluid_sdf_set_filter_kind: " << fluid_last_error() << std::endl;
        return 1;
    }
    if (sim && skind.kind != FLUID_SDF_SURFACE_SPHERES && fluid_sdf_set_surface(sim, &skind) != FLUID_OK) {
        std::cerr << "fluid_sdf_set_surface: " << fluid_last_error() << std::endl;
        return 1;
    }
    if (sim && trails && fluid_sdf_set_trails(sim, &trl) != FLUID_OK) {
        std::cerr << "fluid_sdf_set_trails: " << fluid_last_error() << std::endl;
        return 1;
    }
    if (sim && track && fluid_sdf_set_track(sim, &tk) != FLUID_OK) {
        std::cerr << "fluid_sdf_set_track: " << fluid_last_error() << std::endl;
        return 1;
    }
    if (sim && track_grow && fluid_sdf_set_track_grow(sim, 1) != FLUID_OK) {
        std::cerr << "fluid_sdf_set_track_grow: " << fluid_last_error() << std::endl;
        return 1;
    }
    const bool ref_scene = prm.n == 121 && ppc == 10;   // fluid.cc:1176,1347-1350
    const int32_t flo[3] = {-20, -20, -20}, fhi[3] = {20, 20, 20};
    // fluidGrid of the emitter: the initial cube's box (fluid_scene_water_cube_drop: side round(N 41 / 121), -20..20 at N = 121)
    const int m_src = (int)((double)prm.n * 41.0 / 121.0 + 0.5), c0_src = -(m_src / 2);
    const int32_t slo[3] = {c0_src, c0_src, c0_src}, shi[3] = {c0_src + m_src - 1, c0_src + m_src - 1, c0_src + m_src - 1};
    const int32_t bound_src = -(prm.n / 2) + prm.n - 1;   // 60 at N = 121 (PointList::add's |p| < boundary - 2)
    std::vector<double> src_pos;
    const int64_t np = ref_scene ? fluid_scene_uniform_scatter(flo, fhi, 10.f, (uint32_t)seed, 60, nullptr)
                                 : fluid_scene_water_cube_drop(prm.n, ppc, seed, nullptr);
    std::vector<double> pos((size_t)3 * np);
    if (ref_scene) fluid_scene_uniform_scatter(flo, fhi, 10.f, (uint32_t)seed, 60, pos.data());
    else fluid_scene_water_cube_drop(prm.n, ppc, seed, pos.data());
    if (blocks && *blocks) {
        bc.prm = prm, bc.steps = steps, bc.outdir = outdir, bc.raw_f32 = raw_f32;
        return run_blocks(bc, pos, np, t0);
    }
    if (fluid_upload_particles(sim, np, pos.data(), nullptr) != FLUID_OK) {
        std::cerr << "fluid_upload_particles: " << fluid_last_error() << std::endl;
        return 1;
    }
    if (!outdir.empty()) mkdir(outdir.c_str(), 0755);  // the reference aborts when simulation/ is missing
    const size_t ncell = (size_t)prm.n * prm.n * prm.n;
    std::vector<float> out(outdir.empty() || !out_dense ? 0 : ncell);
    // file.write(grids) of fluid.cc:1508: `grids` is declared outside the loop (:1366) and receives every step's grid
    // (:1450), so the final mygrids.vdb holds all of them — streamed here, one grid appended per step
    fluid_vdb_writer_t* all = nullptr;
    std::string fin;
    if (!outdir.empty() && steps > 0) {
        const size_t slash = outdir.find_last_of('/');   // beside the output directory: ./mygrids.vdb for the default "simulation"
        fin = (slash == std::string::npos ? std::string() : outdir.substr(0, slash + 1)) + "mygrids.vdb";
        if (fluid_vdb_open(fin.c_str(), prm.n, steps, FLUID_VDB_ZIP_ACTIVE_MASK, &all) != FLUID_OK) { std::cerr << "cannot write " << fin << std::endl; return 1; }
    }

    LeafWriter lw;
    const bool leaves = !outdir.empty() && steps > 0 && !out_dense;
    if (leaves) {
        lw.outdir = outdir, lw.fin = fin, lw.all = all, lw.raw_f32 = raw_f32;
        lw.voxel = (float)prm.dx;
        lw.vel_scale = (float)mesh_vel_scale;
        lw.mesh_what = mesh_what;
        lw.start();
    }
    // hands the oldest snapshot to the writer thread
    auto pass_on = [&](int step) {
        fluid_leaf_grid_t g;
        if (fluid_output_wait(sim, &g) != FLUID_OK) {
            std::cerr << "fluid_output_wait: " << fluid_last_error() << std::endl;
            return false;
        }
        fluid_sdf_grid_t sg;
        if (surface && fluid_sdf_wait(sim, &sg) != FLUID_OK) {
            std::cerr << "fluid_sdf_wait: " << fluid_last_error() << std::endl;
            return false;
        }
        fluid_mesh_t mg;
        fluid_mesh_attr_t ma;
        fluid_mesh_ex_t mx{};
        if (mesh && (mesh_more ? fluid_mesh_wait_ex(sim, &mg, &mx) : mesh_vel ? fluid_mesh_wait_attr(sim, &mg, &ma) : fluid_mesh_wait(sim, &mg)) != FLUID_OK) {
            std::cerr << "fluid_mesh_wait: " << fluid_last_error() << std::endl;
            return false;
        }
        fluid_image_t im;
        if (render && fluid_render_wait(sim, &im) != FLUID_OK) {
            std::cerr << "fluid_render_wait: " << fluid_last_error() << std::endl;
            return false;
        }
        lw.submit(step, g, surface ? &sg : nullptr, mesh ? &mg : nullptr, mesh && mesh_vel && !mesh_more ? &ma : nullptr, nullptr, nullptr,
                  mesh && mesh_more ? &mx : nullptr, render ? &im : nullptr);
        return true;
    };

    double dt = prm.max_dt;  // fluid.cc:1367
    double simulationTime = 0;
    for (int i = 0; i < steps; ++i) {
        std::cout << "2" << std::endl;
        std::cout << "3" << std::endl;
        std::cout << "DT " << dt << std::endl;
        std::cout << "Before" << std::endl;
        fluid_step_stats_t st;
        if (fluid_step(sim, &st) != FLUID_OK) {
            std::cerr << "fluid_step: " << fluid_last_error() << std::endl;
            return 1;
        }
        if (src_every > 0 && i % src_every == 0) {   // fluid.cc:1374-1375, 1379, 1495, 1497
            const int64_t ns = fluid_scene_uniform_scatter(slo, shi, 10.f, (uint32_t)(i + 1), bound_src, nullptr);
            src_pos.resize((size_t)3 * (ns > 0 ? ns : 0));
            if (ns < 0 || fluid_scene_uniform_scatter(slo, shi, 10.f, (uint32_t)(i + 1), bound_src, src_pos.data()) != ns ||
                fluid_add_particles(sim, ns, src_pos.data(), nullptr) != FLUID_OK) {
                std::cerr << "fluid_add_particles: " << fluid_last_error() << std::endl;
                return 1;
            }
        }
        std::cout << "After" << std::endl;
        dt = st.dt_out;
        std::cout << "DT " << dt << std::endl;
        std::cout << "Error:\t" << st.error << std::endl;
        std::cout << "Iteration:\t" << i + 1 << std::endl;
        simulationTime += dt;
        std::cout << "Time delta:\t" << simulationTime << std::endl;
        if (src_every > 0) std::cout << "Particles:\t" << fluid_num_particles(sim) << std::endl;
        if (leaves) {
            // snapshot i reuses the slot of grid i - 2: that grid must be on disk
            if (!lw.wait_done(i - 1)) { std::cerr << "cannot write " << lw.error << std::endl; lw.stop(); return 1; }
            if (fluid_output_snapshot(sim) != FLUID_OK) {
                std::cerr << "fluid_output_snapshot: " << fluid_last_error() << std::endl;
                lw.stop();
                return 1;
            }
            if (trails_dt) {   // SHUTTER = dt: the path of the step just taken
                trl.shutter = st.dt_out;
                if (fluid_sdf_set_trails(sim, &trl) != FLUID_OK) {
                    std::cerr << "fluid_sdf_set_trails: " << fluid_last_error() << std::endl;
                    lw.stop();
                    return 1;
                }
            }
            if (surface && (smooth ? fluid_sdf_snapshot_filtered(sim, &sp, &sf) : fluid_sdf_snapshot(sim, &sp)) != FLUID_OK) {
                std::cerr << "fluid_sdf_snapshot: " << fluid_last_error() << std::endl;
                lw.stop();
                return 1;
            }
            if (mesh && (mesh_more ? fluid_mesh_snapshot_ex(sim, &mp, smooth ? &sf : nullptr, mesh_what)
                         : mesh_vel ? fluid_mesh_snapshot_attr(sim, &mp, smooth ? &sf : nullptr)
                         : smooth ? fluid_mesh_snapshot_filtered(sim, &mp, &sf)
                                  : fluid_mesh_snapshot(sim, &mp)) != FLUID_OK) {
                std::cerr << "fluid_mesh_snapshot: " << fluid_last_error() << std::endl;
                lw.stop();
                return 1;
            }
            if (render && fluid_render_snapshot(sim, &rp, smooth ? &sf : nullptr, &rcam, nullptr, FLUID_RENDER_RGB) != FLUID_OK) {
                std::cerr << "fluid_render_snapshot: " << fluid_last_error() << std::endl;
                lw.stop();
                return 1;
            }
            if (i > 0 && !pass_on(i - 1)) { lw.stop(); return 1; }   // its copy ran beside this step
        } else if (!outdir.empty()) {
            if (fluid_download_field(sim, FLUID_FIELD_OUTPUT, out.data(), ncell * sizeof(float)) != FLUID_OK) {
                std::cerr << "fluid_download_field: " << fluid_last_error() << std::endl;
                return 1;
            }
            // file2.write(grids2) of fluid.cc:1503-1504: simulation/mygrids<i>.vdb.  grids2 is declared inside the loop
            // (:1373), so each of these files holds exactly the grid of its step.
            const std::string fn = outdir + "/mygrids" + std::to_string(i) + ".vdb";
            const float* gp[1] = {out.data()};
            if (fluid_write_vdb(fn.c_str(), prm.n, 1, gp) != FLUID_OK) { std::cerr << "cannot write " << fn << std::endl; return 1; }
            if (fluid_vdb_append(all, out.data()) != FLUID_OK) { std::cerr << "cannot write " << fin << std::endl; return 1; }
            if (raw_f32) {
                const std::string fr = outdir + "/mygrids" + std::to_string(i) + ".f32";
                if (!write_f32(fr, prm.n, out.data(), ncell)) { std::cerr << "cannot write " << fr << std::endl; return 1; }
            }
        }
    }
    if (leaves) {
        const bool ok = pass_on(steps - 1) && lw.wait_done(steps);
        lw.stop();
        if (!ok) {
            if (!lw.error.empty()) std::cerr << "cannot write " << lw.error << std::endl;
            return 1;
        }
    }
    if (all && fluid_vdb_close(all) != FLUID_OK) { std::cerr << "cannot write " << fin << std::endl; return 1; }
    fluid_destroy(sim);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "Time Taken " << sec / 60 << " minutes" << std::endl;  // fluid.cc:1513 (wall, not clock())
    return 0;
}
