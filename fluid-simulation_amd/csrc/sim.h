// Internal state of a handle and the host functions shared by fluid_api.hip (one GPU) and fluid_dist.hip (decomposed runs).
#pragma once
#include "common.h"
#include "../../include/fluid_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

int fluid_fail(int code, const std::string& msg);   // sets fluid_last_error() of the calling thread, returns code
#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return fluid_fail(FLUID_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
    } while (0)
#include "snap_ring.h"   // the two-slot hand-off of the snapshots (uses HIPCHK)

using namespace fl;

struct ProfClass {
    long launches = 0, sampled = 0;
    double ms = 0, cells = 0;
    std::vector<hipEvent_t> e0, e1;
    std::vector<double> pc;
};

struct fluid_sim {
    fluid_params_t prm;
    Grid g;
    size_t ncell = 0;
    hipStream_t st = nullptr;
    // grid fields
    uint8_t *solid = nullptr, *flags = nullptr;
    float *container = nullptr, *rhs = nullptr, *diver = nullptr, *diver2 = nullptr;
    double *u = nullptr, *v = nullptr, *w = nullptr, *ub = nullptr, *vb = nullptr, *wb = nullptr;
    double *dcx = nullptr, *dcy = nullptr, *dcz = nullptr, *pressure = nullptr;
    double* p_guess = nullptr;    // last solved pressure, never cleared: the multigrid PCG starts from it (solve_start = FLUID_START_ZERO: from 0 like the reference)
    bool warm = true, have_guess = false;
    // Passes of one step's do..while solve the SAME matrix for right-hand sides b_{k+1} = (1 - f) b_k + c (f = update_frac: the partial
    // velocity update takes f of the pressure gradient out of the divergence, c = what gravity puts back, the same in every pass), so
    // p_{k+1} = p_k + (1 - f)(p_k - p_{k-1}) up to the float32 rounding of b: from the third pass on the solve starts from that.
    double* p_guess2 = nullptr;   // the solution before p_guess
    long guess_step = -1, guess2_step = -1;   // step counter and pass index at which each was stored
    int guess_pass = -1, guess2_pass = -1;
    long step_counter = 0;
    bool extrapolate = true;      // FLUID_EXTRAPOLATE=0 switches it off
    // the start of this solve: guess arrays and coefficients (g2 == nullptr: plain warm start); called by both solve paths
    // ... and q = p_{k+1} - (1 - f) p_k = A^-1 c changes little from one step to the next (c is gravity's share; the walls and most of the
    // water stay where they are): kept from the last step that ran two passes (p_q, make_q), it starts the SECOND pass of a step from
    // (1 - f) p_0 + q — 23 -> 21 iterations with q = 0, -> 18-19 with the last q in the splash of the 256^3 drop.  (The FIRST pass of the
    // next step from (1 - f) p_last + q: measured, no fewer iterations.)
    double* p_q = nullptr;
    long q_step = -1;
    void start_guess(const double*& g1, const double*& g2, double& ca, double& cb) const
    {
        g1 = p_guess, g2 = nullptr, ca = 1.0, cb = 0.0;
        const int k = stats.outer_passes;   // passes completed in this step = index of this one
        const bool same_step = p_guess2 && k >= 2 && guess_step == step_counter && guess2_step == step_counter && guess_pass == k - 1 && guess2_pass == k - 2;
        const double f = 1.0 - prm.update_frac;
        if (extrapolate && same_step) {
            g2 = p_guess2, ca = 1.0 + f, cb = -f;
        } else if (extrapolate && p_q && q_step >= 0 && step_counter - q_step <= 4 && k == 1 && guess_step == step_counter && guess_pass == 0) {
            g2 = p_q, ca = f, cb = 1.0;
        }
    }
    // right after the second pass of a step (and, in a decomposed run, after its halo exchange): is q to be formed from p_guess, p_guess2?
    bool make_q() const { return warm && p_q && stats.outer_passes == 1 && guess_step == step_counter && guess_pass == 1 && guess2_step == step_counter && guess2_pass == 0; }
    // after store_pressure wrote the new solution into p_guess2's buffer: it becomes the latest
    void rotate_guess()
    {
        std::swap(p_guess, p_guess2);
        guess2_step = guess_step, guess2_pass = guess_pass;
        guess_step = step_counter, guess_pass = stats.outer_passes;
    }
    int *indices = nullptr, *scan_sums = nullptr, *ipart = nullptr;
    // pcg
    void *R = nullptr, *S[2] = {nullptr, nullptr}, *Q = nullptr, *X = nullptr, *Zmg = nullptr;
    double *pcx = nullptr, *pcy = nullptr, *pcz = nullptr;  // getVelocity(c, vels) per cell: allocated on first use, PIC blend only  // box-local layout (LBox)
    uint8_t* cntL = nullptr;
    LBox L{};
    size_t lmax = 0;
    double *part_bb = nullptr, *part_rr = nullptr, *part_rz[2] = {nullptr, nullptr}, *part_pq = nullptr, *part_err = nullptr;
    PcgState* ps = nullptr;
    PcgState* h_ps = nullptr;  // pinned, 2 slots
    hipEvent_t ev_poll[2] = {nullptr, nullptr};
    // particles
    long np = 0, cap = 0;
    Particles pa{}, pb{};
    int *key = nullptr, *slot = nullptr, *order = nullptr, *order2 = nullptr, *cell_count = nullptr, *cell_start = nullptr;
    uint32_t* spid = nullptr;   // original ids in sorted-position order (per-cell rank pass)
    double *stage_pos = nullptr, *stage_vel = nullptr;
    double* pw = nullptr;  // 9 axis weights per particle, SoA with stride cap
    double* p2g_part = nullptr;  // k_p2g_rows' three x-plane partials: 12 doubles per cell of the P2G box (grown on demand)
    size_t p2g_part_cap = 0;
    int2* p2g_crowd = nullptr;   // (cell, piece) list of k_p2g_crowd_sum, grown on demand; its count is p2g_items[1]
    size_t p2g_crowd_cap = 0;
    int* p2g_items = nullptr;    // k_p2g_rows' work list (count + int4 items), grown on demand; the count is 0 between launches
    size_t p2g_items_cap = 0;
    int max_cell = 0;            // most particles in one cell after the last sort (all ranks' cells when distributed)
    // mostly-air box (splash, settled pool): level-0 legs, SQ and XR run over compacted lists of the tiles that hold an unknown
    uint8_t* tl_flags = nullptr;  // per-tile flags (both tile shapes, one after the other)
    int *tl_mg = nullptr, *tl_sq = nullptr;
    size_t tl_cap = 0;
    int n_tl_mg = 0, n_tl_sq = 0;
    int *row_flags = nullptr, *row_pos = nullptr, *row_list = nullptr;   // XR's list of non-empty z rows (32 cells), built with the tile lists
    size_t row_cap = 0;
    int n_rows = 0;
    bool rows_on = true;          // XR over the z rows that hold an unknown (finer than the SQ tile list)
    // closed pockets (airborne droplets) of the pressure system, solved on their own (kernels_droplets.hip; FLUID_DROPLETS=0: off)
    bool drops_on = true;
    bool row_sweeps = true;       // FLUID_ROW_SWEEPS=0: the per-step box sweeps keep their cell-per-thread forms (kernels_grid.hip, k_*4)
    int* drop_ctr = nullptr;      // 64 x DROP_NCTR ints: the slot counters, then DROP_NCTR + 1 range starts of the dense numbering
    int* drop_n = nullptr;        // cells per component
    int* drop_cells = nullptr;    // 64 local-box cell indices per component
    int n_drop = 0;               // components taken out of this step's global solve
    int drop_last = -1;           // ... found by the last search (-1: none yet); below drop_min the search runs every 8th step only
    int drop_min = 4000;          // FLUID_DROPLETS_MIN (measured at 256^3: the search pays from ~4 000 droplets on)
    int drop_skipped = 0;
    bool lists_hint = false;      // the previous step's box was mostly air: build the lists before this step's flags sync
    bool lists_on = false;        // this step's solves use them
    int lists_force = -1;         // FLUID_TILE_LISTS=0|1
    int p2g_force = 0;           // FLUID_P2G_FORM=rows|tiles: 1 / 2, for experiments
    long p2g_ref_cells = 0;      // decomposed run: cells of the GLOBAL active box (0: use Rb)
    long last_num_active = 0;    // unknowns of the previous step (the same on every rank)
    StepState* ss = nullptr;
    StepState* h_ss = nullptr;  // pinned
    // boxes
    Box Pb{0, 0, 0, -1, -1, -1}, Rb{0, 0, 0, -1, -1, -1}, Sb{0, 0, 0, -1, -1, -1};
    Box dirty{0, 0, 0, -1, -1, -1};   // box holding non-zero step-field data (zeroed before the next P2G)
    int flag_x0 = 0, flag_x1 = -1;    // x planes whose flags / indices the last flags pass may have made non-trivial
    bool flags_valid = false;         // flags / indices outside [flag_x0, flag_x1] are known to be "solid or empty" / -1
    bool sorted = false, have_p2g = false, have_flags = false;
    long n_out = 0;           // particles whose base cell is off the grid (last bucket of the sorted array), from the last sort
    bool sort_hint = false;   // Pb is the bounding box of THESE particles one step ago (false after an upload)
    // One GPU: FLIPadvect's kernel also bins the positions it writes (k_advect_bin), and the box, off-grid count and fullest
    // cell come back with the read that ends the step: the next sort starts at its scan, with no pass over the positions, no
    // copy and no wait.  `binned` holds while key, slot, cell_count (the planes bin_x0..bin_x1 and the tail buckets) describe
    // the particles as they are now; whatever touches the particles, their count, p_off or those arrays in between clears it.
    bool advect_bin = true;       // FLUID_ADVECT_BIN=0: k_advect alone, every sort bins for itself
    bool binned = false;
    int bin_x0 = 0, bin_x1 = -1;  // x planes of cell_count zeroed before the binning
    int bin_min[3] = {0, 0, 0}, bin_max[3] = {-1, -1, -1}, bin_n_out = 0, bin_max_cell = 0;   // what k_bin_bbox would have found
    // the first poll of a multigrid PCG solve also carries the rest of the pressure pass, guarded by the solve's done flag
    bool solve_tail = true;       // FLUID_SOLVE_TAIL=0: the tail is enqueued after the poll
    bool tail_ran = false;        // solve_mg: this pass's vel_update, rhs_div(1) and err_norm ran, *h_ss holds the pass error
    double dt = 0.1;
    fluid_step_stats_t stats{};
    // multigrid preconditioner (single-GPU fp64 solve)
    static constexpr int MG_MAXL = 8;
    int mg_nl = 0, mg_tail = 0;   // levels; first level handled by the single-block tail kernel
    // iteration count of the previous multigrid solve of the same kind (sizes the first unpolled batch): first pass of a step, second pass,
    // later passes (those start from the extrapolation and need about half the iterations)
    long mg_last_iters_k[3] = {0, 0, 0};
    int pass_class() const { return stats.outer_passes < 2 ? stats.outer_passes : 2; }
    int mg_csweeps = 3;           // red-black sweeps (each direction) on the coarsest level (12 -> 2 changes the PCG count by 1 in 520)
    MLevel mgl[MG_MAXL];
    uint8_t *mg_typ[MG_MAXL] = {}, *mg_cnt[MG_MAXL] = {};
    // Galerkin coarse levels by aggregation (kernels_gal.hip): mostly-air boxes, float cycle, one GPU.  FLUID_MG_GALERKIN=0|1
    int gal_mode = 1;             // FLUID_MG_GALERKIN: 0 never, 1 whichever cycle needed fewer iterations when last measured (mostly-air boxes), 2 always there
    int gal_it[2] = {-1, -1};     // first-pass iterations of the last step that used the re-discretised / the Galerkin cycle (-1: not measured)
    int gal_since_probe = 0;      // steps since the worse cycle was last looked at
    bool gal_eligible = false;    // this step could have taken the Galerkin cycle
    bool gal = false;             // ... and in use this step (set by mg_setup)
    int gal_lc = 0;               // the coarsest level of the Galerkin cycle (one block)
    double gal_dt = 0;            // dt the coefficients were built with
    double gal_wc = 1.8;          // over-correction of the piecewise-constant prolongation 
    int gal_sweeps = 3;           // red-black sweeps, each direction, on the coarsest level (2 ... 16: the same iteration counts)
    char* gal_slab = nullptr;     // per level 1..gal_lc: gd, gx, gy, gz (float) and the unknown flags
    size_t gal_slab_cap = 0;
    float* gal_c[MG_MAXL][4] = {};
    uint8_t* gal_cnt[MG_MAXL] = {};
    uint8_t* gal_tfl[MG_MAXL] = {};   // per leg tile: holds an unknown
    char *mg_u[MG_MAXL] = {}, *mg_v[MG_MAXL] = {}, *mg_f[MG_MAXL] = {}, *mg_r[MG_MAXL] = {};  // per level: u, ping-pong, rhs, residual (float or double)
    double mg_wc[4] = {1.25, 1.1, 1.0, 1.0};   // weight of the coarse correction at level 0 / level 1 / deeper kernel levels / inside the tail 
    bool mg_fp32 = true;           // the V-cycle computes and stores in float inside the double PCG (mg_precision = FLUID_MG_FP64: double)
    double* mg_part = nullptr;    // per-block partials of r.z when a level-0 launch has more blocks than the PCG kernels re-sum
    char* mg_slab = nullptr;      // one allocation behind every mg_* array and Zmg (re-carved each step)
    size_t mg_slab_cap = 0;
    // multi-GPU (3-D block decomposition, fluid_dist.hip)
    bool dist = false;
    struct DistState* ds = nullptr;
    long p_off = 0;              // my live particles are pa[p_off .. p_off+np)
    int* d_small = nullptr;      // device scratch ints
    int* h_small = nullptr;      // pinned mirror
    // particle sources and sinks (fluid_sources.hip), applied at the end of fluid_step when any slot is set.  Boxes are global
    // index boxes, a slot's buffer is box-sized and holds nothing that depends on the window: re-balancing hands it on as it is.
    struct SrcSlot {
        bool on = false;
        bool mask_ok = false;   // decomposed: the buffer's solid bytes are those of the scene (fluid_set_solid clears it)
        fluid_source_t src{};
        Box box{};
        int* buf = nullptr;     // carved by source_buf
    };
    SrcSlot src[FLUID_MAX_SOURCES];
    Box sink[FLUID_MAX_SINKS] = {};
    bool sink_on[FLUID_MAX_SINKS] = {};
    int* src_sums = nullptr;      // block sums of the scans over a box or over the particles (any count up to INT32_MAX)
    long n_steps = 0;             // fluid_step calls completed: the t of the sources
    bool vel_ok = false;          // u, v, w are the velocities a completed step left (fluid_add_particles with vel == NULL)
    long src_emit_last = 0, src_rm_last = 0, src_emit_total = 0, src_rm_total = 0;
    struct OutState* out = nullptr;   // leaf snapshots of the output grid (fluid_output.hip), made by the first fluid_output_snapshot
    int out_every = 0;                // fluid_dist_output_every: fluid_step snapshots the owned block at the end of step t iff t % every == 0
    struct SdfState* sdf = nullptr;   // level-set snapshots of the particles (fluid_sdf.hip): slots, streams and scratch of their own
    struct MeshState* mesh = nullptr; // surface-net snapshots of that level set (fluid_mesh.hip): slots, stream and per-leaf scratch of their own
    struct RenderState* render = nullptr;   // ray-cast images of that level set (fluid_render.hip): slots, stream and per-leaf scratch of their own
    // profiling
    int prof_every = 0;
    ProfClass prof[FLUID_PROF_COUNT];
};

namespace fl {
inline bool box_empty(const Box& b) { return b.x1 < b.x0 || b.y1 < b.y0 || b.z1 < b.z0; }
Box clip_dilate(const Box& b, int d, const Grid& g);      // dilate by d cells, clipped to the window
template <typename T>
inline hipError_t dalloc(T** p, size_t n)
{
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(T));
    return e;
}
// scratch that is sized again: the old array goes first (hipFree waits for the device, so whoever still reads it has ended)
template <typename T>
inline hipError_t regrow(T*& p, size_t n)
{
    if (p) hipFree(p);
    p = nullptr;
    return hipMalloc((void**)&p, n * sizeof(T));
}
inline int grid_leaves(const Grid& g) { return ((g.hi & ~7) - (g.lo & ~7)) / 8 + 1; }   // OpenVDB's 8^3 leaves that meet [lo, hi], per axis
// entry of a call that works on one kind of handle only (one GPU, or with want_dist a decomposed one): `why` says what the
// other kind lacks and what to call instead
inline int snap_guard(const fluid_sim* s, const char* why, bool want_dist = false)
{
    if (!s) return fluid_fail(FLUID_ERR_ARG, "null handle");
    return s->dist != want_dist ? fluid_fail(FLUID_ERR_STATE, why) : FLUID_OK;
}
constexpr const char* ATTR_SINGLE = "these surface attribute calls are single-GPU only: a decomposed handle gives a rank record with squared distances (fluid_dist_sdf_snapshot_attr) and the records merge on the host (fluid_sdf_attr_grids_merge)";
inline size_t solver_elem(const fluid_sim* s) { return s->prm.precision == FLUID_PRECISION_FP32 ? 4 : 8; }
inline bool use_mg(const fluid_sim* s) { return s->prm.preconditioner == FLUID_PRECOND_MG && s->prm.precision == FLUID_PRECISION_FP64; }

int prof_begin(fluid_sim* s, int k, double cells);
void prof_end(fluid_sim* s, int k, int tok);
int alloc_particles(fluid_sim* s, long n);
int grow_particles(fluid_sim* s, long need);
int read_ss(fluid_sim* s);
int sort_pass(fluid_sim* s, int ax0, int ax1, int* h_tail = nullptr);   // counting sort over the x planes [ax0, ax1] of the window
int clear_dirty(fluid_sim* s);
int run_p2g(fluid_sim* s, const Box& box);
template <typename T>
Coef<T> make_coef(const fluid_sim* s);
MgCoef<double> mg_coef(const fluid_sim* s, int level);
hipError_t zero_search(fluid_sim* s, size_t lb);
int phase_flags(fluid_sim* s);
int phase_pressure_pass(fluid_sim* s, double* error);
int pic_fields(fluid_sim* s);
int fluid_create_window(const fluid_params_t* p, const Grid& g, fluid_sim_t** out);   // fluid_create on a window of the grid

// fluid_sources.hip: one GPU's step, and what it shares with dist_sources_apply and the fluid_dist_set_* entry points
int sources_apply(fluid_sim* s);     // end of fluid_step: the sinks, then the sources in slot order (no launch when none is set)
void sources_free(fluid_sim* s);
void sources_move(fluid_sim* from, fluid_sim* to);   // re-balance: slots, sinks, scan scratch and counters go to the new window's handle
extern const char* const SRC_SINGLE;   // snap_guard texts of the one-GPU / the decomposed entry points
extern const char* const SRC_DIST;
int source_set(fluid_sim* s, int32_t slot, const fluid_source_t* src);   // bodies of the entry points, behind the guards
int sink_set(fluid_sim* s, int32_t slot, const int32_t lo[3], const int32_t hi[3]);
int source_stats(const fluid_sim* s, int64_t* emitted_last, int64_t* removed_last, int64_t* emitted_total, int64_t* removed_total);
// a slot's buffer: FILL histogram | kept per cell | its scan | kept per owned cell | its scan | the box's solid bytes.  One GPU
// holds the first three only (cnt_own == nullptr, off_own == off, mask == nullptr)
struct SrcBuf {
    int *hist, *cnt, *off, *cnt_own, *off_own;
    uint8_t* mask;
};
SrcBuf source_buf(const fluid_sim* s, const fluid_sim::SrcSlot& q);
struct SrcDue {   // a due slot at step t: what its launches take
    const fluid_sim::SrcSlot* q;
    SrcBuf a;       // cnt_own == nullptr, off_own == off also where a rank owns the whole box
    uint64_t h0;    // sm(sm(seed) ^ t)
    bool fill;
    OwnBox ob;
    SolidView sv;
};
SinkSet sinks_on(const fluid_sim* s);
SrcDue source_due(const fluid_sim* s, const fluid_sim::SrcSlot& q, long t, const OwnBox& ob);
int source_count(fluid_sim* s, const SrcDue& u);                     // FILL: the histogram of this handle's live particles (enqueued)
int source_plan(fluid_sim* s, const SrcDue& u, long* m, long* mo);   // plan, scan(s), read-back: the box's new points / this handle's
int source_room(fluid_sim* s, long mo);
void source_emit(fluid_sim* s, const SrcDue& u, Particles p, uint32_t id0);
void source_widen_Pb(fluid_sim* s, const Box& b);
void sources_tally(fluid_sim* s, long emitted, long removed);

// fluid_output.hip
void output_free(fluid_sim* s);      // waits for the copies in flight, frees the staging and pinned buffers
int output_auto_check(fluid_sim* s); // entry of fluid_step: FLUID_ERR_STATE when this step's own snapshot would be the third outstanding
int output_auto(fluid_sim* s);       // after FLIPadvect of step t = n_steps: the snapshot of fluid_dist_output_every, when due
void output_move(fluid_sim* from, fluid_sim* to);   // re-balance: slots, counters, `every` and the step count go to the new window's handle

// fluid_sdf.hip
void sdf_free(fluid_sim* s);         // waits for the copies in flight, frees the scratch, the staging and the pinned buffers
void sdf_move(fluid_sim* from, fluid_sim* to);      // re-balance: slots, streams, scratch and counters go to the new window's handle
// the front half of a level-set snapshot, for fluid_sdf_snapshot and fluid_mesh_snapshot alike
struct SdfFront {
    SdfGeom g;
    bool any;             // some particle counts: g holds the box and the range, tv / flags are filled for every leaf of the range
    const float* tv;      // 512 values per leaf of the range (stale where flags[j] == 0): the filter's last buffer when filt is set
    const int* flags;     // the leaf's values are valid (the search's listed flag, or what the last dilation left); what the mesh and the ray caster read by
    const int* list;      // the leaf is listed: flags, or after a tracked filter's trim the flags derived from what the trim left
    int track_n;          // "liquid surface, renormalised": the handle's setting, copied by sdf_begin when a filter is given:
    bool track_trim;      // passes per track and the trim; 0 / false: the filter runs untracked
    int track_scheme;     // FLUID_SDF_TRACK_FIRST_BIAS or FLUID_SDF_TRACK_HJWENO5: which kernel a normalisation pass launches
    bool grow;            // "liquid surface, grown band": every track begins with a dilation, and the range is dilate + T cells
    int kind;             // "liquid surface, flows": the handle's FLUID_SDF_FILTER_* setting, copied by sdf_begin (width rule checked there)
    const fluid_sdf_filter_t* filt;   // nullptr: unfiltered.  Set by sdf_begin from its argument (limits checked there)
    int dilate;           // cells the base-cell box is dilated by for the range: 4; 5 for a filtered mesh (set by the caller after sdf_begin); with grow sdf_front adds T
    bool attr;            // "liquid surface, attributes": the search also keeps the closest particle (set by the caller after sdf_begin)
    const uint64_t* tm;   // 8 mask words per leaf of the range (stale where flags[j] == 0)
    const uint32_t* tid;  // attr: 512 ids per leaf of the range, and
    const float* tvel;    // [leaf][axis][512] velocities (both stale where flags[j] == 0; nullptr without attr)
    bool dist2;           // with attr: the search also writes m per voxel (set by the caller after sdf_begin)
    const float* tmin;    // dist2: 512 per leaf of the range, m where active and +inf elsewhere (stale where flags[j] == 0)
    bool averaged;        // "liquid surface, averaged positions": the handle's fluid_sdf_set_surface setting, copied by sdf_begin,
    float h2, ih2;        // and its constants; sdf_front refuses it together with attr
    bool record;          // "averaged positions (decomposed runs)": the search writes the rank record (dist2 into tmin, the sums) and no
                          // tv / tm; set by the caller after an sdf_begin that was handed the surface
    bool trails;          // "liquid surface, velocity trails": the handle's fluid_sdf_set_trails setting is on, copied by sdf_begin (never
                          // with a surface handed in); sdf_front bins the particles' instances and refuses it together with attr
    fluid_sdf_trails_t tr;   // trails: the setting's copy, or the trails handed in
    bool trails_arg;      // "velocity trails (decomposed runs)": the trails were handed in (spheres, whatever the handle's settings say);
                          // sdf_front passes over the dead entries of a decomposed handle and keeps the rank record's counters
};
// limits of the parameters (and of the filter, when one is given), the state, the constants of g.  sf: nullptr = the handle's
// fluid_sdf_set_surface setting; otherwise the surface is this one (checked by the caller) and the setting is not read.  tr: nullptr =
// the handle's fluid_sdf_set_trails setting; otherwise spheres and these trails (limits checked by the caller), no setting is read
int sdf_begin(fluid_sim* s, const fluid_sdf_params_t* p, SdfFront* f, const fluid_sdf_filter_t* filt = nullptr,
              const fluid_sdf_surface_t* sf = nullptr, const fluid_sdf_trails_t* tr = nullptr);
int sdf_front(fluid_sim* s, SdfFront* f);   // bbox (waits for the stream) -> count, scan, scatter -> search -> the filter's passes and tracks

// fluid_mesh.hip
void mesh_free(fluid_sim* s);        // waits for the copies in flight, frees the scratch, the staging and the pinned buffers

// fluid_render.hip
void render_free(fluid_sim* s);      // waits for the copies in flight, frees the scratch, the staging and the pinned buffers

// fluid_dist.hip
int dist_step(fluid_sim* s, fluid_step_stats_t* stats);
void dist_destroy(fluid_sim* s);
int dist_download_field(fluid_sim* s, int field, void* dst, size_t bytes, bool* handled);
void dist_keep_solid(fluid_sim* s, const uint8_t* solid_global);
}  // namespace fl
