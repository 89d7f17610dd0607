/*
 * fluid_hip.h — C ABI of the MI355X-native PIC/FLIP step (libfluid_hip.so).
 *
 * The reference (Aakash1312/Fluid-Simulation) has no plugin/FFI interface: the hot path is
 * the body of the step loop in main() (fluid.cc:1368-1507).  This header is the boundary a
 * maintainer would bind instead of that loop body; every entry point names the reference
 * lines it replaces.  Plain pointers and sizes only; no C++ or torch types; no exceptions
 * cross the boundary (int status, fluid_last_error() for the text).
 *
 * Conventions
 *   grid      N cells per axis, cell coordinate c in [lo,hi], lo = -(N/2), hi = lo+N-1
 *             (N=121 -> the reference's -60..60, fluid.cc:1159).  "W" = [lo+2,hi-2]
 *             (the reference's literal 58, fluid.cc:1264).  Dense layout, z fastest:
 *             linear = ((x-lo)*N + (y-lo))*N + (z-lo)  — the order of the reference's
 *             index numbering sweep (fluid.cc:1416-1433).
 *   particles host side AoS xyz doubles, like std::vector<openvdb::Vec3d> (fluid.cc:806-807).
 *   ownership device memory belongs to the handle; host buffers belong to the caller.
 *   threading one handle = one host thread = one HIP stream; calls are sequential.
 */
#ifndef FLUID_HIP_H
#define FLUID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fluid_sim fluid_sim_t;

/* status codes */
#define FLUID_OK 0
#define FLUID_ERR_ARG 1      /* bad argument                                   */
#define FLUID_ERR_HIP 2      /* HIP runtime error (no device, OOM, launch)     */
#define FLUID_ERR_STATE 3    /* call order (e.g. step before upload_particles) */
#define FLUID_ERR_SOLVER 4   /* PCG hit the iteration cap / broke down         */
#define FLUID_ERR_PEER 5     /* multi-GPU: another rank failed in this step; every rank returns together */

/* field ids for fluid_download_field / fluid_upload_field */
#define FLUID_FIELD_CONTAINER 0   /* float32 N^3  particle weight density (fluid.cc:1157,1413)        */
#define FLUID_FIELD_WEIGHTS 1     /* float32 N^3  P2G weights (fluid.cc:809,1108); == container here (grazing addends) */
#define FLUID_FIELD_VEL 2         /* float64 3*N^3, SoA planes [u|v|w] (Vec3dGrid vels, :1240)        */
#define FLUID_FIELD_VEL_BEFORE 3  /* float64 3*N^3  velBeforeUpdate (:1455)                           */
#define FLUID_FIELD_INDICES 4     /* int32   N^3   unknown numbering, -1 elsewhere (:1388,1416-1433)  */
#define FLUID_FIELD_RHS 5         /* float32 N^3   rhs grid of the last setRHS (:1234,414-479)        */
#define FLUID_FIELD_DIVER 6       /* float32 N^3   b of the last pass = diver grid (:1231,566-610)    */
#define FLUID_FIELD_PRESSURE 7    /* float64 N^3   p scattered back to cells (VectorXd p, :1474)      */
#define FLUID_FIELD_OUTPUT 8      /* float32 N^3   outputGrid written to .vdb (:1434-1448)            */
#define FLUID_FIELD_SOLID 9       /* uint8   N^3   1 = solid (:1166,1266)                             */
#define FLUID_FIELD_DIVER2 14     /* float32 N^3   b2, divergence after the update (:1477-1481)       */
#define FLUID_FIELD_SEARCH 15     /* solver dtype N^3  PCG search vector s (stencil input)            */
#define FLUID_FIELD_Q 16          /* solver dtype N^3  q = A s (stencil output)                       */
#define FLUID_FIELD_FLAGS 17      /* uint8   N^3   bit0 solid, bit1 fluid, bits2-4 diag count         */

/* solver precision */
#define FLUID_PRECISION_FP64 0    /* fp64 PCG vectors (reference arithmetic: Eigen VectorXd)          */
#define FLUID_PRECISION_FP32 1    /* fp32 PCG vectors (stencil micro-benchmark / experiments only)    */

/* preconditioner of the PCG (fluid_params.preconditioner); the reference uses Eigen IncompleteCholesky */
#define FLUID_PRECOND_MG 0        /* geometric multigrid V(2,2) cycle; iteration count independent of N  */
#define FLUID_PRECOND_JACOBI 1    /* Eigen DiagonalPreconditioner arithmetic, iteration-for-iteration Eigen's Jacobi CG */

/* start of every pressure solve (fluid_params.solve_start) */
#define FLUID_START_WARM 0        /* x0 = the previous solve's pressure (Eigen's solveWithGuess form of the same loop;
                                     the converged p is the same within cg_tol, cg_iters is NOT the reference's count);
                                     from the third pass of a step's do..while on: x0 = p_k + (1 - update_frac)(p_k - p_{k-1}),
                                     exact up to the float32 rounding of the right-hand side (same matrix, b_{k+1} = 0.9 b_k + c) */
#define FLUID_START_ZERO 1        /* x0 = 0 like the reference's cg.solve(b), fluid.cc:1474: cg_iters comparable        */

/* arithmetic of the multigrid V-cycle inside the fp64 PCG (fluid_params.mg_precision) */
#define FLUID_MG_FP32 0           /* float cycle (default: M^-1 only has to be a fixed SPD operator)     */
#define FLUID_MG_FP64 1           /* double cycle                                                        */

/* multi-GPU pressure block (fluid_params.dist_solve; fluid_create_dist only) */
#define FLUID_DIST_AUTO 0         /* decomposed solve when the active box is large, replicated otherwise */
#define FLUID_DIST_DECOMPOSED 1   /* domain-decomposed PCG with the globally coupled V-cycle             */
#define FLUID_DIST_REPLICATED 2   /* P2G fields all-reduced, the pressure block solved on every rank     */

typedef struct fluid_params {
    int32_t n;                /* cells per axis                         fluid.cc:1159 (121)      */
    int32_t device;           /* HIP device ordinal                                             */
    double dx;                /* cell size                              fluid.cc:1358 (1.0)      */
    double rho;               /* density                                fluid.cc:1471,1475 (1)   */
    double gravity[3];        /*                                        fluid.cc:1357 (0,-10,0)  */
    double max_dt;            /* maxTimeStep of FLIPadvect              fluid.cc:1490 (0.1)      */
    double outer_tol;         /* do..while(error > 0.1)                 fluid.cc:1484            */
    double update_frac;       /* velUpdate(dt/10)                       fluid.cc:1475 (0.1)      */
    double cg_tol;            /* Eigen default epsilon                  IterativeSolverBase.h:283 */
    int32_t cg_max_iters;     /* 0 = 2*numActive                        IterativeSolverBase.h:362 */
    int32_t max_outer_passes; /* 0 = unlimited (reference)                                       */
    int32_t precision;        /* FLUID_PRECISION_*                                               */
    int32_t preconditioner;   /* FLUID_PRECOND_*                                                  */
    double flip_blend;        /* 1 = pure FLIP (the reference, fluid.cc:981); b < 1 blends in the PIC gather of
                                 the reference's unused clampedCatmullRom (fluid.cc:125-207):
                                 v' = b (v + delta) + (1-b) v_pic.  Build extension.      */
    int32_t solve_start;      /* FLUID_START_*                                                   */
    int32_t mg_precision;     /* FLUID_MG_*                                                      */
    int32_t dist_solve;       /* FLUID_DIST_*                                                    */
    int32_t pad_;             /* must be 0                                                       */
} fluid_params_t;

typedef struct fluid_step_stats {
    double dt_in;             /* dt used by this step's pressure block  fluid.cc:1469-1475       */
    double dt_out;            /* dt written by FLIPadvect               fluid.cc:992-999         */
    double error;             /* last ||b-b2||/||b||                    fluid.cc:1483            */
    double max_speed;         /*                                        fluid.cc:976-991         */
    double relres;            /* last solve: sqrt(|r|^2/|b|^2)          ConjugateGradient.h:87   */
    int64_t num_active;       /* numActive                              fluid.cc:1395-1433       */
    int32_t outer_passes;     /* passes of the do..while                fluid.cc:1457-1484       */
    int32_t cg_iters;         /* PCG iterations summed over the passes                           */
    int32_t cg_iters_last;    /* iterations of the last solve                                    */
    int32_t box_lo[3];        /* active box of this step (index space, inclusive)                */
    int32_t box_hi[3];
    int32_t paths;            /* kernel forms this step took: FLUID_PATH_* bits                  */
} fluid_step_stats_t;
#define FLUID_PATH_P2G_TILES 1   /* particle -> grid in its 2 x 2-column tile form (a box whose row partials would not fit) */
#define FLUID_PATH_P2G_CROWD 16  /* particle -> grid with the cells of >= 18 particles summed on the matrix cores first (piled particles, mostly empty box) */
#define FLUID_PATH_TILE_LISTS 2  /* level-0 solver kernels over the lists of tiles that hold an unknown (mostly-air box) */
#define FLUID_PATH_DIST_DECOMPOSED 4  /* multi-GPU: window arrays, domain-decomposed PCG with the globally coupled V-cycle  */
#define FLUID_PATH_DIST_REPLICATED 8  /* multi-GPU: particles sharded, pressure block replicated on every rank              */
#define FLUID_PATH_DIST_REBALANCED 32 /* multi-GPU: the cut planes were moved at the end of this step (the window changed)      */
#define FLUID_PATH_MG_GALERKIN 128   /* the V-cycle's coarse levels were Galerkin operators by aggregation (mostly-air box whose re-discretised levels lose much of the pool) */
#define FLUID_PATH_DROPLETS 64        /* closed pockets of <= 64 unknowns (airborne droplets) were solved apart from the global system   */
#define FLUID_PATH_DROPLETS_SHORT 256 /* ... and at least one of them left its own CG by the iteration cap or a breakdown, not by the stopping rule (relres above cg_tol there) */
#define FLUID_PATH_G2P_TILES 1024     /* one GPU: grid -> particle gathered through LDS tiles (k_g2p_tiled ran: sorted, densely filled, non-empty base-cell box); else thread per particle */

/* ---- lifetime ------------------------------------------------------------------------- */
/* Reference defaults (N=121, g=(0,-10,0), dx=1, rho=1, max_dt=0.1, outer_tol=0.1,
 * update_frac=0.1, cg_tol=2.2e-16, fp64).  fluid.cc:1357-1367. */
int fluid_default_params(fluid_params_t* p);
/* Allocates all device fields, sets the default solid shell (solid outside W,
 * fluid.cc:1256-1266).  Replaces the grid/PointList set-up of fluid.cc:1157-1347. */
int fluid_create(const fluid_params_t* p, fluid_sim_t** out);
int fluid_destroy(fluid_sim_t* s);
/* Text of the last error on the calling thread ("" if none). */
const char* fluid_last_error(void);
/* "libfluid_hip <version> gfx950" */
const char* fluid_version(void);

/* ---- scene ---------------------------------------------------------------------------- */
/* solid[N^3] uint8, 1 = solid (saccessor.setValue(xyz,1), fluid.cc:1266,1341).  Cells outside
 * W must be solid (the reference reads pressure(-1) otherwise) -> FLUID_ERR_ARG. */
int fluid_set_solid(fluid_sim_t* s, const uint8_t* solid);
/* PointList contents (fluid.cc:806-807,841): n particles, pos/vel = 3n doubles AoS.
 * vel may be NULL (zeros, like PointList::add). */
int fluid_upload_particles(fluid_sim_t* s, int64_t n, const double* pos, const double* vel);
/* Back to the caller in the ORIGINAL upload order. */
int fluid_download_particles(fluid_sim_t* s, double* pos, double* vel);
int64_t fluid_num_particles(fluid_sim_t* s);
/* dt carried between steps (double dt, fluid.cc:1367; written by FLIPadvect :1490). */
int fluid_set_dt(fluid_sim_t* s, double dt);
int fluid_get_dt(fluid_sim_t* s, double* dt);
/* Host-only synthetic input "water_cube_drop" (generalises fluid.cc:1176,1349 +
 * PointScatter.h:421-429): centred cube of side round(N*41/121) cells, ppc particles per cube
 * voxel at c - 0.5 + U[0,1)^3 (counter-based RNG).  pos==NULL -> returns the count only.
 * Needs no GPU. */
int64_t fluid_scene_water_cube_drop(int32_t n, int32_t ppc, uint64_t seed, double* pos);
/* Host-only: the reference's own initial particles — what
 *   fluidGrid->fill(CoordBBox(lo, hi), 0, true); std::mt19937 r(seed);
 *   UniformPointScatter<PointList, std::mt19937>(pos, points_per_volume, r)(*fluidGrid);      fluid.cc:1176,1347-1350
 * leaves in PointList::positions (openvdb/tools/PointScatter.h:143-185, tree fill + ValueOn order, libstdc++'s mt19937 /
 * uniform_int / uniform_real, g++'s right-to-left argument evaluation), with PointList::add's |p| < boundary - 2 filter
 * (fluid.cc:841; boundary <= 0: none).  The reference's scene: lo = -20, hi = 20, 10.f, seed 0, boundary 60 -> 689210
 * points for a 121^3 grid.  pos == NULL -> returns the count only; < 0 on bad arguments.  Needs no GPU. */
int64_t fluid_scene_uniform_scatter(const int32_t lo[3], const int32_t hi[3], float points_per_volume, uint32_t seed,
                                    int32_t boundary, double* pos);

/* ---- the step ------------------------------------------------------------------------- */
/* One iteration of the loop body fluid.cc:1378-1490 (everything except the .vdb write). */
int fluid_step(fluid_sim_t* s, fluid_step_stats_t* stats);

/* Per-phase entry points (parity tests drive these one by one). */
int fluid_p2g(fluid_sim_t* s);                 /* fluid.cc:1378,1384 (P2Gtransfer 1106-1148) + 1388-1413 (interpolate 843-882) */
int fluid_flags_index(fluid_sim_t* s);         /* fluid.cc:1416-1455 index sweep, output copy, velBeforeUpdate */
int fluid_rhs_div(fluid_sim_t* s, int which);  /* setRHS+setDiver: which=0 -> b (1469-1470), 1 -> b2 (1477-1480) */
int fluid_solve(fluid_sim_t* s);               /* setA,setA2,compute,solve fluid.cc:1471-1474 (matrix-free PCG) */
int fluid_vel_update(fluid_sim_t* s);          /* velUpdate(dt/10) fluid.cc:1475 */
int fluid_pressure_pass(fluid_sim_t* s, double* error); /* one do..while body fluid.cc:1457-1483 */
int fluid_flip_advect(fluid_sim_t* s);         /* FLIPadvect fluid.cc:1490 (972-1038) */
/* Stats of the phases run since the last fluid_step / fluid_p2g. */
int fluid_get_stats(fluid_sim_t* s, fluid_step_stats_t* stats);

/* ---- fields --------------------------------------------------------------------------- */
/* bytes must equal the field's size (see FLUID_FIELD_*). */
int fluid_download_field(fluid_sim_t* s, int field, void* dst, size_t bytes);
/* Upload CONTAINER (then call fluid_flags_index), VEL, VEL_BEFORE, DIVER, PRESSURE, SEARCH. */
int fluid_upload_field(fluid_sim_t* s, int field, const void* src, size_t bytes);

/* ---- the reference's unused grid / particle utilities --------------------------------------------
 * `extrapolate` (fluid.cc:705-802) and `PointList::resample` (fluid.cc:1053-1080) are dead code in the reference — the one
 * call of extrapolate, at the end of P2Gtransfer (fluid.cc:1147), is commented out and resample is never called — so fluid_step
 * does not run them; they are here for a caller that wants the reference's code path with them switched on.  Single GPU.
 * fluid_extrapolate: call after fluid_p2g; fills FLUID_FIELD_VEL (and VEL_BEFORE) of every cell inside W that P2G left without
 * a velocity with the average of its defined 26-neighbours, layer by layer; n_layers (may be NULL) = passes RUN — the "anything new"
 * counter is read back every 8 passes, so this is the number of layers that filled a cell rounded up to a multiple of 8.
 * fluid_resample: at most per_cell particles per base cell, in upload-index order; the others are parked at
 * (hi + 40, hi + 40, hi + 40) (the reference's (100, 100, 100)); only cells with x < hi - 10 (its `rx < 50`). */
int fluid_extrapolate(fluid_sim_t* s, int32_t* n_layers);
int fluid_resample(fluid_sim_t* s, int32_t per_cell, int64_t* n_parked);

/* ---- particle sources and sinks (single GPU; SURVEY 8(f): the reference's commented-out emitter) ----------------------
 * The reference builds a UniformPointScatter over fluidGrid every step (fluid.cc:1374-1375) and has its call, with
 * pos.interpFromGrid(vels, 60, containerGrid) after it, commented out after FLIPadvect (fluid.cc:1495-1497; also under
 * `if (i%5 == 0)` at :1379-1382).  fluid_add_particles is that call; persistent sources and sinks are its general form, applied
 * by fluid_step itself at the end of every step, after FLIPadvect: first every sink, then every source in slot order.
 * A decomposed handle (fluid_create_dist) returns FLUID_ERR_STATE from every entry point of this block: it uses the
 * fluid_dist_* entry points of the next block, which keep global particle ids across the ranks.
 *
 * Where a source puts its points (a fixed function of seed, t, cell and k; SplitMix64):
 *   sm(x):  z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *           return z ^ z >> 31                                                        (all uint64, wrapping)
 *   for step t (0-based fluid_step count of the handle), cell c (linear index of the Conventions block) and point k of it:
 *   key = sm(sm(sm(seed) ^ t) ^ linear) ^ k;  u_a = (sm(key + a) >> 11) * 2^-53 (a = 0, 1, 2);  p_a = c_a + (u_a - 0.5)
 * A cell is eligible if it lies in the box, inside W and is not solid; a point is kept iff round(p) == c on all three axes.
 * Kept points take pids np, np+1, ... in ascending (linear, k) order. */
#define FLUID_MAX_SOURCES 8
#define FLUID_MAX_SINKS 8
#define FLUID_SOURCE_ADD 0        /* per_cell new points in every eligible cell                                       */
#define FLUID_SOURCE_FILL 1       /* top every eligible cell up to per_cell particles (counted by base cell round(p))  */
#define FLUID_SOURCE_VEL_FIXED 0  /* new points take vel[]                                                            */
#define FLUID_SOURCE_VEL_GRID 1   /* new points take interpFromGrid's velocity (see fluid_add_particles)              */
#define FLUID_PATH_SOURCES 512    /* fluid_step_stats.paths: a sink or a source changed the particle set this step    */
typedef struct fluid_source {
    int32_t lo[3], hi[3];   /* inclusive cell box (index space of the Conventions block: 0 .. N-1)                   */
    int32_t per_cell;       /* 1..64                                                                                 */
    int32_t mode;           /* FLUID_SOURCE_ADD / FLUID_SOURCE_FILL                                                  */
    int32_t every;          /* emit at the end of step t iff t % every == 0 (>= 1)                                   */
    int32_t vel_mode;       /* FLUID_SOURCE_VEL_FIXED / FLUID_SOURCE_VEL_GRID                                        */
    double vel[3];
    uint64_t seed;
} fluid_source_t;
/* Appends n particles (AoS xyz doubles, like fluid_upload_particles) after the live ones, with pids np .. np+n-1, so that
 * fluid_download_particles returns the old particles and then the new ones.  vel == NULL is the reference's interpFromGrid
 * (fluid.cc:883-894): each new particle's velocity is clampedCatmullRom (fluid.cc:125-207) at its position over the grid velocities
 * of the last completed fluid_step (after the update), averaged to cell centres as getVelocity does (fluid.cc:58-70); cells outside
 * W are skipped, (0,0,0) when the weights sum to 0; FLUID_ERR_STATE when no step has completed since the last upload.
 * The warm start of the solve is kept. */
int fluid_add_particles(fluid_sim_t* s, int64_t n, const double* pos, const double* vel);
/* slot in [0, FLUID_MAX_SOURCES); src == NULL clears the slot.  FLUID_ERR_ARG on an empty or off-grid box, per_cell outside
 * 1..64, a bad mode or vel_mode, every < 1. */
int fluid_set_source(fluid_sim_t* s, int32_t slot, const fluid_source_t* src);
/* slot in [0, FLUID_MAX_SINKS); lo == NULL clears the slot.  At the end of every step each particle whose base cell round(p) lies
 * in the inclusive box [lo, hi] is removed; the others keep their order and are renumbered 0 .. np'-1. */
int fluid_set_sink(fluid_sim_t* s, int32_t slot, const int32_t lo[3], const int32_t hi[3]);
/* Particles added by the sources / removed by the sinks in the last step, and in all steps since the handle was created
 * (fluid_add_particles is not counted).  Any pointer may be NULL. */
int fluid_get_source_stats(fluid_sim_t* s, int64_t* emitted_last, int64_t* removed_last, int64_t* emitted_total, int64_t* removed_total);

/* ---- particle sources and sinks of a decomposed run (handles of fluid_create_dist, both pressure modes) ------------------
 * The same slots, limits, modes, argument checks and point formula as above, for every rank of a block-decomposed run.  A
 * fluid_create handle gets FLUID_ERR_STATE from these four (it uses the entry points above), as a decomposed handle does there.
 * Boxes are GLOBAL index boxes, `linear` is the global linear index (x*N + y)*N + z, solid is the global mask.  The set calls
 * are collective in the sense of fluid_dist_set_rebalance: every rank of the run sets the same slots before the same step.
 *
 * When.     Inside fluid_step, after FLIPadvect and before the automatic output snapshot and the re-balancing (new particles
 *           are counted and routed like any others), with t = the handle's count of completed steps, which re-balancing keeps.
 *           First every sink, then the sources in slot order.
 * Sinks.    A live particle whose base cell round(p) lies in a sink box is removed on whichever rank holds it at the end of
 *           the step (after advect that may be one cell outside its holder's block).  It is marked dead where it is; nothing is
 *           compacted.  THE SURVIVORS KEEP THEIR IDS: ids are never renumbered on a decomposed run.  This is the one deliberate
 *           difference from the one-GPU step, whose sinks renumber the pids 0 .. np'-1.
 * Sources.  Eligible cells, tries per cell and kept points are those of the one-GPU definition.  FILL counts the live
 *           particles per cell over ALL ranks after the sinks (one SUM all-reduce of the box-sized histogram per FILL source
 *           that is due).  A kept point is created on the rank that owns its cell, with id next_id + j, j = its rank in ascending
 *           (linear, k) order over the whole box; then next_id += m.  Every rank plans and scans the whole box (it keeps a copy
 *           of the global solid mask over the box for that), so the ids need no exchange.  next_id starts as 1 + the largest id
 *           any rank was ever handed (fluid_upload_particles_ids, fluid_dist_add_particles; tracked per handle, agreed by one
 *           MAX all-reduce in each step where a source is due) and only grows.  If next_id + m would reach 0xFFFFFFFF (the mark of
 *           a dead particle) every rank returns FLUID_ERR_STATE before that source writes anything.
 *           So: the particles of all ranks sorted by id are the sequence fluid_download_particles gives on one GPU with the
 *           same slots, as long as the uploaded ids were 0 .. np-1 (survivors in pid order, then the new points by slot, linear, k).
 * Velocity. FLUID_SOURCE_VEL_GRID and fluid_dist_add_particles(vel == NULL) give interpFromGrid's velocity, bit for bit the
 *           one-GPU value: the ranks exchange a 1-wide halo of the cell-centre averages (decomposed mode), so the latter call is
 *           collective there — every rank calls it, n = 0 is fine.  Velocities outside the step's box are zero, as on one GPU.
 * Cost.     A step with no sink set and no source due adds no launch, no transport call and no wait.  Otherwise: one SUM
 *           all-reduce of the removed count (sinks set), one MAX all-reduce of next_id (a source due), per due FILL source the
 *           histogram's all-reduce, per emitting source one agreement (below) and, with FLUID_SOURCE_VEL_GRID in decomposed mode,
 *           one halo exchange.
 * Failure.  Growing the particle arrays for emitted points can fail on one rank alone: every rank then leaves the step, that one
 *           with its own error, the others with FLUID_ERR_PEER (agreed before the next transport call).
 * Re-balancing carries the slots, the counters and next_id into the new windows. */
int fluid_dist_set_source(fluid_sim_t* s, int32_t slot, const fluid_source_t* src);   /* NULL clears */
int fluid_dist_set_sink(fluid_sim_t* s, int32_t slot, const int32_t lo[3], const int32_t hi[3]);   /* lo == NULL clears */
/* Global numbers, the same on every rank; FLUID_PATH_SOURCES is set on every rank when the global particle set changed. */
int fluid_dist_get_source_stats(fluid_sim_t* s, int64_t* emitted_last, int64_t* removed_last, int64_t* emitted_total, int64_t* removed_total);
/* Appends the caller's points with the caller's ids (unique ids are the caller's job; 0xFFFFFFFF is not an id).  Every point's
 * base cell must lie in this rank's block (an edge block reaches to infinity on its outer sides), else FLUID_ERR_ARG and nothing
 * is appended (checked on the host).  vel == NULL needs a step completed on this window (FLUID_ERR_STATE otherwise, also right
 * after a step that moved the cut planes). */
int fluid_dist_add_particles(fluid_sim_t* s, int64_t n, const double* pos, const double* vel, const uint32_t* ids);

/* The closed pockets of the last step's pressure system that were solved apart from the global solve (FLUID_PATH_DROPLETS;
 * kernels_droplets.hip): n_components of them; cells (may be NULL) receives 64 entries per component — the window-array cell
 * indices (ix * ny + iy) * nz + iz of its unknowns, ascending, padded with -1 — for at most cap_components components. */
int fluid_get_droplets(fluid_sim_t* s, int32_t* n_components, int64_t* cells, int32_t cap_components);

/* ---- stencil operator alone (micro-benchmark + parity of the 7-point apply) ------------ */
/* q = A s with the matrix of fluid.cc:304-412 for the current flags and dt; `reps` launches
 * timed with HIP events on the handle's stream; avg_ms = mean duration of one launch.
 * box: 0 = dense sweep over all N^3 cells, 1 = active box only. */
int fluid_stencil_apply(fluid_sim_t* s, int reps, int box, float* avg_ms);
/* The same, HBM-proof: the launches rotate over `nsets` separate copies of (s, q, flags), as many as `footprint_bytes` needs
 * (one set = (2 T + 1) N^3 bytes; at least 2), so that with a footprint well above the 256 MiB Infinity Cache no launch
 * finds its operands cached — fluid_stencil_apply's back-to-back launches over ONE set of 151 MB (fp32, 256^3) do.
 * nsets_out: the number of sets used.  q of the last launch is left in the handle's FLUID_FIELD_Q. */
int fluid_stencil_apply_hbm(fluid_sim_t* s, int reps, int box, int64_t footprint_bytes, int32_t* nsets_out, float* avg_ms);

/* ---- known-answer hooks ------------------------------------------------------------------- */
/* w[i] = spline(x[i]) (fluid.cc:22-37) evaluated by the DEVICE function the P2G / G2P kernels use (which = 0), or the
 * three-cell form those kernels call per axis, spline_at(p, round(p) - 1 + d, d) with d = which - 1 (which = 1..3: x[i]
 * is then the particle coordinate p).  Host buffers; tests compare bit for bit with the reference's own function. */
int fluid_spline_eval(int32_t device, int32_t which, int64_t n, const double* x, double* w);
/* out[0] = sum_i a[i] * b[i] over n doubles with the block-partial + fixed-order re-summation the PCG kernels use for
 * their dot products (restates the long dot-product test of openvdb/unittest/TestConjGradient.cc:212-237). */
int fluid_dot_eval(int32_t device, int64_t n, const double* a, const double* b, double* out);
/* The exclusive prefix sum the sort and the unknown numbering use, over n elements that start in_offset / out_offset elements
 * (0..64) behind an aligned device address, as the sort passes cell_count + c0.  mode 0: in = n int32, out[i] = in[0] + .. +
 * in[i-1]; mode 1: in = n flag bytes, out[i] = the count of fluid bytes before i where byte i is fluid, -1 elsewhere.
 * *total = the sum over all n.  Fails when anything outside out[0, n) was written.  Host buffers. */
int fluid_scan_eval(int32_t device, int32_t mode, int64_t n, int32_t in_offset, int32_t out_offset, const void* in, int32_t* out, int32_t* total);

/* ---- profiling ------------------------------------------------------------------------- */
/* Kernel classes timed with hipEvent pairs on the handle's stream. */
#define FLUID_PROF_PCG_SQ 0      /* fused p-update + 7-point apply + dot     */
#define FLUID_PROF_PCG_XR 1      /* fused x,r update + dots                  */
#define FLUID_PROF_P2G 2
#define FLUID_PROF_G2P 3
#define FLUID_PROF_SORT 4
#define FLUID_PROF_SOLVE 5       /* whole solve                              */
#define FLUID_PROF_MG_UP0 6  /* level-0 up leg of the V-cycle (k_mg_up)      */
#define FLUID_PROF_COUNT 7
/* Every `sample_every`-th launch of the per-iteration classes (PCG_SQ, PCG_XR, MG_UP0) and every max(1, sample_every / 8)-th
 * launch of the per-step classes (P2G, G2P, SORT, SOLVE) is bracketed by an event pair (0 = off).  An event record stalls the
 * stream by ~5-10 us: sample sparsely inside a timed region. */
int fluid_profile_enable(fluid_sim_t* s, int sample_every);
/* Resolves pending events; n_launches = launches seen, n_sampled = launches timed,
 * total_ms = sum over the timed ones, cells = sum of cells swept by the timed ones. */
int fluid_profile_read(fluid_sim_t* s, int klass, int64_t* n_launches, int64_t* n_sampled, double* total_ms, double* cells);
int fluid_profile_reset(fluid_sim_t* s);

/* ---- multi-GPU: 3-D block decomposition (one process per GPU) --------------------------------
 * The reference is single-process (no communication backend); this is new design
 * (SURVEY.md 8e).  The grid is cut into dims[0] x dims[1] x dims[2] blocks by per-axis cut planes;
 * rank r owns block (bx, by, bz) = (r / (dims[1] dims[2]), (r / dims[2]) % dims[1], r % dims[2]):
 * its cells, and the particles whose base cell (round(pos), fluid.cc:267) lies in it.
 *
 *   decomposed solve   a rank's field arrays cover its block + a 4-cell halo ring only (the
 *                      "window").  Per step: particle migration and ghost particles with the
 *                      <= 26 adjacent blocks, halo exchanges of flags / velocity / pressure /
 *                      FLIP delta, the unknown numbering from all-reduced row counts, and a
 *                      domain-decomposed PCG whose multigrid V-cycle is globally coupled: halo
 *                      exchanges of the residual and of the coarse correction inside the two
 *                      finest levels, the coarser levels gathered (one all-reduce) and solved
 *                      redundantly on every rank — the same cycle as on one GPU, so the
 *                      iteration count does not grow with the number of blocks.
 *   replicated solve   particles sharded the same way, but every rank keeps full-size arrays;
 *                      the P2G result of the active box is assembled on every rank by one SUM
 *                      all-reduce and the pressure block runs identically everywhere (bit-identical
 *                      to the one-GPU step; fallback for boxes too small to be worth exchanging).
 *
 * Transport is supplied by the caller (RCCL inside the library: fluid_rccl_comm_create; gloo in
 * the tests: the Python callbacks; an in-process transport for several blocks per process:
 * fluid_local_comm_create).  All pointers are DEVICE pointers; calls must be ordered after prior
 * work on `stream` and complete (or be stream-ordered) before later work on it.  Return 0 on
 * success.  Every rank makes the same sequence of allreduce calls; exchange calls are matched
 * pairwise (rank a lists peer b with the byte counts b lists for a, in both directions). */
#define FLUID_DT_F64 0
#define FLUID_DT_I32 1
#define FLUID_DT_I64 2
#define FLUID_DT_F32 3
#define FLUID_DT_U8 4
#define FLUID_OP_SUM 0
#define FLUID_OP_MAX 1
#define FLUID_OP_MIN 2
#define FLUID_MAX_RANKS 64
typedef struct fluid_comm {
    int32_t rank, size;
    void* ctx;
    /* Neighbour exchange: for i < n send sbytes[i] bytes from sbuf[i] to rank peer[i] and receive
     * rbytes[i] bytes from the same rank into rbuf[i] (either count may be 0).  Peers are distinct. */
    int (*exchange)(void* ctx, int32_t n, const int32_t* peer, const void* const* sbuf, const size_t* sbytes,
                    void* const* rbuf, const size_t* rbytes, void* stream);
    /* In-place all-reduce of `count` elements of dtype FLUID_DT_* with FLUID_OP_*. */
    int (*allreduce)(void* ctx, void* buf, int64_t count, int32_t dtype, int32_t op, void* stream);
} fluid_comm_t;

/* Native transport: fluid_comm_t over RCCL (grouped ncclSend/ncclRecv, ncclAllReduce on the solver's stream).
 * librccl_path: the librccl.so to dlopen ("" = by name); id128: ncclUniqueId made by rank 0 with
 * fluid_rccl_unique_id and handed to the other ranks by the launcher.  Binds to the current HIP device. */
int fluid_rccl_unique_id(const char* librccl_path, void* id128);
int fluid_rccl_comm_create(const char* librccl_path, const void* id128, int32_t rank, int32_t size, fluid_comm_t* out);
int fluid_rccl_comm_destroy(fluid_comm_t* comm);
const char* fluid_rccl_last_error(void);

/* In-process transport: `size` handles driven by `size` host threads of ONE process (several blocks per GPU: the
 * tests run 2 x 2 x 2 blocks on the one GPU of their box this way; a host that drives several GPUs from one
 * process can use it too).  Device-to-device copies between the handles' buffers, host-side rendezvous. */
int fluid_local_group_create(int32_t size, void** group);
int fluid_local_group_destroy(void* group);
/* Wakes every rank waiting inside the transport with an error: the driver thread of a rank that failed elsewhere calls it. */
int fluid_local_group_abort(void* group);
int fluid_local_comm_create(void* group, int32_t rank, fluid_comm_t* out);

typedef struct fluid_decomp {
    int32_t dims[3];          /* blocks per axis; dims[0]*dims[1]*dims[2] == comm->size                        */
    const int32_t* cuts[3];   /* cuts[a][0..dims[a]]: cuts[a][0] = 0, cuts[a][dims[a]] = n, ascending; interior
                                 cuts are multiples of 4 and every block is >= 8 cells wide (the coupled V-cycle
                                 coarsens 2 x 2 x 2 twice across block faces)                                  */
} fluid_decomp_t;
/* Like fluid_create, for rank comm->rank of comm->size. */
int fluid_create_dist(const fluid_params_t* p, const fluid_comm_t* comm, const fluid_decomp_t* decomp, fluid_sim_t** out);
/* Geometry of this handle's arrays in a decomposed run (one GPU: the whole grid): global index of the window's first
 * cell, window dims (the shape of fluid_download_field's arrays), owned block [own_lo, own_hi) in global indices. */
int fluid_window(fluid_sim_t* s, int32_t origin[3], int32_t dims[3], int32_t own_lo[3], int32_t own_hi[3]);
/* Upload THIS rank's particles (base cell inside its block) with their global ids (unique
 * across ranks; the order of fluid_download_particles_ids is the device order). */
int fluid_upload_particles_ids(fluid_sim_t* s, int64_t n, const double* pos, const double* vel, const uint32_t* ids);
/* This rank's current particles and ids; call with NULLs to get the count. */
int64_t fluid_download_particles_ids(fluid_sim_t* s, double* pos, double* vel, uint32_t* ids);
/* Cut planes for dims[0] x dims[1] x dims[2] blocks of about equal particle count per axis slab, from a host
 * particle set (host-only); cuts[a] receives dims[a]+1 values that satisfy fluid_decomp's rules. */
int fluid_partition_blocks(int32_t n, int64_t np, const double* pos, const int32_t dims[3], int32_t* cuts_x, int32_t* cuts_y,
                           int32_t* cuts_z);
/* Re-balancing of the cut planes of a decomposed run: every `every` steps (0 = never, the default) the blocks' particle counts
 * are compared and, when the fullest holds more than `ratio` x the mean (>= 1), the planes are placed anew by particle count and
 * the particles handed to their new owners; collective — every rank of the run sets the same values.  The window of this handle
 * then changes (fluid_window), fields downloaded afterwards have the new shape, and the step that did it reports
 * FLUID_PATH_DIST_REBALANCED.  fluid_dist_get_cuts: the current planes (dims[a] + 1 values per axis) and how often they moved. */
int fluid_dist_set_rebalance(fluid_sim_t* s, int32_t every, double ratio);
int fluid_dist_get_cuts(fluid_sim_t* s, int32_t* cuts_x, int32_t* cuts_y, int32_t* cuts_z, int32_t* n_rebalanced);
/* What a decomposed handle decided about itself (any pointer may be NULL): overlap = 0 not checked yet (no solve with peers so far),
 * 1 the residual's overlapped halo exchange (second stream) delivered the serial exchange's bytes on every rank and is in use,
 * 2 it did not on some rank and is switched off everywhere; cg_form = 0 two scalar all-reduces per PCG iteration, 1 Chronopoulos-Gear
 * (one); n_refused = re-balances every rank gave up together because some rank could not build its second window. */
int fluid_dist_get_info(fluid_sim_t* s, int32_t* overlap, int32_t* cg_form, int32_t* n_refused);

/* ---- OpenVDB file output (replaces file2.write(grids2) / file.write(grids), fluid.cc:1503-1504,1508) ----
 * Dense float32 N^3 arrays (z fastest, cell (0,0,0) = index coordinate (lo,lo,lo), lo = -(N/2)) written as unnamed
 * FloatGrids (Tree_float_5_4_3, background 0, voxel size 1, every cell of [lo,hi]^3 active) in OpenVDB's file format 224
 * — the grids fluid.cc:1161-1164,1434-1451 builds.  Host only: no GPU, no OpenVDB library (zlib for the ZIP flag).
 * The reference writes ONE grid into every simulation/mygrids<i>.vdb (`grids2` lives inside the loop, fluid.cc:1373) and
 * EVERY step's grid into the final mygrids.vdb (`grids`, :1366,1450,1508): the streaming form appends one grid per step. */
#define FLUID_VDB_ACTIVE_MASK 2       /* io/Compression.h:80 COMPRESS_ACTIVE_MASK                                  */
#define FLUID_VDB_ZIP_ACTIVE_MASK 3   /* COMPRESS_ZIP | COMPRESS_ACTIVE_MASK: the library's default (Compression.h:78-81) */
typedef struct fluid_vdb_writer fluid_vdb_writer_t;
int fluid_vdb_open(const char* path, int32_t n, int32_t n_grids, int32_t compression, fluid_vdb_writer_t** out);
int fluid_vdb_append(fluid_vdb_writer_t* w, const float* grid);     /* exactly n_grids times                       */
int fluid_vdb_close(fluid_vdb_writer_t* w);                         /* FLUID_ERR_ARG if fewer grids were appended  */
/* n_grids arrays in one call; fluid_write_vdb = ZIP | ACTIVE_MASK. */
int fluid_write_vdb(const char* path, int32_t n, int32_t n_grids, const float* const* grids);
int fluid_write_vdb_ex(const char* path, int32_t n, int32_t n_grids, const float* const* grids, int32_t compression);

/* ---- output as non-zero leaves (single GPU) ------------------------------------------------------------------------------
 * The density grid of a step is mostly +0 (a falling cube fills ~ 5 % of OpenVDB's 8^3 leaves, a settled pool ~ 15 %), and the
 * file needs every leaf all the same (fill([lo,hi]^3, 0, active), fluid.cc:1163).  So the grid leaves the device as the list of
 * its leaves that hold anything else, and the writer produces from that list the bytes it produces from the dense array.
 * Leaves are OpenVDB's: origins at multiples of 8 in index space (lo = -(N/2): for N = 121 the first leaf starts at -64 and holds
 * 4 in-grid cells per axis).  A leaf is listed iff an in-grid voxel of it has a non-zero BIT PATTERN (-0.0f and NaN count).
 *
 *   fluid_step(s, &st);  fluid_output_snapshot(s);            enqueue only: the next fluid_step overlaps the copy
 *   fluid_step(s, &st);  fluid_output_wait(s, &g);            g = the grid of the FIRST step
 *   fluid_vdb_append_leaves(writers, 2, &g);                  may run on another host thread: it reads g's pointers only
 * A decomposed run takes its grid out block by block with the next section ("output as non-zero leaves (decomposed runs)").
 */
typedef struct fluid_leaf_grid {
    int32_t n;               /* cells per axis of the grid the leaves belong to                                  */
    int32_t n_leaves;
    const int32_t* origin;   /* 3 per leaf: index-space origin, multiples of 8, ascending (x, y, z)               */
    const float* values;     /* 512 per leaf, ((x&7)*8 + (y&7))*8 + (z&7); voxels outside [lo,hi]^3 hold +0       */
} fluid_leaf_grid_t;
#define FLUID_OUTPUT_LEAF_BYTES (2048 + 12)   /* what a listed leaf costs on the way to the host: 512 floats + its origin  */
#define FLUID_OUTPUT_HEADER_BYTES 4           /* ... and the count of listed leaves, once per snapshot                     */
/* Captures FLUID_FIELD_OUTPUT as it is at the call: mark, scan and pack kernels on the handle's stream (ordered before the next
 * step clears the grid), the count of listed leaves read back (4 bytes), then the packed records copied to pinned host memory on a
 * second stream — not waited for here.  Two snapshots may be outstanding; a third returns FLUID_ERR_STATE.  Buffers belong to the
 * handle, grow on demand here (never inside a step) and are freed by fluid_destroy after the copies in flight have ended.
 * A decomposed handle (fluid_create_dist) returns FLUID_ERR_STATE from these three entry points. */
int fluid_output_snapshot(fluid_sim_t* s);
/* The oldest snapshot not yet waited for (FLUID_ERR_STATE when there is none); a grid of zeros has n_leaves = 0 and NULL
 * pointers.  The pointers stay valid until the SECOND following fluid_output_snapshot on the handle. */
int fluid_output_wait(fluid_sim_t* s, fluid_leaf_grid_t* out);
/* Of the last snapshot (any pointer may be NULL): bytes_to_host = leaves_listed * FLUID_OUTPUT_LEAF_BYTES + FLUID_OUTPUT_HEADER_BYTES. */
int fluid_output_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host);
/* Host only: dense[n^3] (z fastest) = +0 everywhere, then the in-grid voxels of every listed leaf.  FLUID_ERR_ARG on a bad list
 * (see fluid_vdb_append_leaves). */
int fluid_leaves_to_dense(const fluid_leaf_grid_t* g, float* dense);
/* Appends the grid `g` describes to each of n_writers open writers (same n and compression as g->n / each other).
 * The bytes appended are those fluid_vdb_append writes for fluid_leaves_to_dense(g); the listed leaves are compressed once for
 * all writers of the call, every other leaf's bytes are constants of the writer.  FLUID_ERR_ARG on an origin that is
 * not a multiple of 8, lies outside the leaves of [lo,hi]^3, or is not strictly ascending; FLUID_ERR_STATE on a full writer
 * (nothing is then written to any of them).  Host only. */
int fluid_vdb_append_leaves(fluid_vdb_writer_t* const* writers, int32_t n_writers, const fluid_leaf_grid_t* g);
int fluid_write_vdb_leaves(const char* path, const fluid_leaf_grid_t* g, int32_t compression);

/* ---- output as non-zero leaves (decomposed runs) ---------------------------------------------------------------------------
 * The same list, per block: every rank lists the GLOBAL leaves that meet its owned block [own_lo, own_hi) (fluid_window) and have
 * an owned, in-grid voxel with a non-zero bit pattern.  Origins are global index-space coordinates, ascending (x, y, z); a record
 * is the leaf's 512 floats in the leaf's own voxel order, with +0 in EVERY voxel this rank does not own (halo cells of its window,
 * other ranks' cells — in replicated mode the rest of its full-size array — and voxels outside [lo,hi]^3).  A leaf that a cut plane
 * splits is therefore listed by each rank that owns a non-zero voxel of it, and the ranks' records of it have disjoint support:
 * fluid_leaf_grids_merge ORs them, exactly.  Rank-local: no transport call is made, moving the lists to one place is the caller's
 * (plain host arrays with global origins).
 *
 *   fluid_dist_output_every(s, 1);                                     once, the same on every rank
 *   per step, every rank:    fluid_step(s, &st);  fluid_dist_output_wait(s, &part[rank]);
 *   one place:               k = fluid_leaf_grids_merge(part, R, cap, origin, values);
 *                            g = {n, k, origin, values};  fluid_vdb_append_leaves(writers, 2, &g);
 */
/* Captures the owned block of FLUID_FIELD_OUTPUT as it is at the call; otherwise fluid_output_snapshot in every respect: kernels on
 * the handle's stream, the 4-byte count read back, the records copied on a second stream and not waited for, two snapshots may be
 * outstanding (a third: FLUID_ERR_STATE), buffers grow here.  A plain fluid_create handle is accepted: its owned block is the
 * grid, the list is fluid_output_snapshot's, and both forms share the handle's two slots and its count of outstanding snapshots. */
int fluid_dist_output_snapshot(fluid_sim_t* s);
/* The oldest snapshot not yet waited for, as fluid_output_wait; out->n is the global N.  The pointers stay valid until the SECOND
 * following snapshot on the handle — also across a step that moves the cut planes (FLUID_PATH_DIST_REBALANCED): the list is then
 * still the old window's block. */
int fluid_dist_output_wait(fluid_sim_t* s, fluid_leaf_grid_t* out);
/* leaves_in_block = global leaves that meet the owned block now; the other two of the last snapshot:
 * bytes_to_host = leaves_listed * FLUID_OUTPUT_LEAF_BYTES + FLUID_OUTPUT_HEADER_BYTES.  Any pointer may be NULL. */
int fluid_dist_output_stats(fluid_sim_t* s, int64_t* leaves_in_block, int64_t* leaves_listed, int64_t* bytes_to_host);
/* every = 0 (default): off.  every >= 1: fluid_step itself takes the snapshot at the end of every step t with t % every == 0, t = the
 * 0-based count of fluid_step calls on the handle (kept when the planes move): after FLIPadvect and BEFORE the re-balancing, so the
 * grid of a step that moves the planes is captured from the old window (afterwards the fields of the new one are zero).  A step that
 * would take the third outstanding snapshot returns FLUID_ERR_STATE at once, before any work and any transport call.  Every rank of
 * a run sets the same `every` and waits alike (as for fluid_dist_set_rebalance): a rank refused alone leaves its peers in the step. */
int fluid_dist_output_every(fluid_sim_t* s, int32_t every);
/* Host only.  The union of the parts' leaves, ascending (x, y, z), into origin[3 * cap_leaves] / values[512 * cap_leaves]; a leaf that
 * several parts list receives the bitwise OR of their records.  For the lists fluid_dist_output_wait gives on the ranks of a run this
 * is the list fluid_output_snapshot gives for the assembled grid.  Returns the merged leaf count (origin == values == NULL: the count
 * only, cap_leaves is ignored), or -FLUID_ERR_ARG with nothing written: n_parts < 1, the parts' n differ, a part breaks the list
 * rules of fluid_vdb_append_leaves, two parts hold a non-zero bit pattern for the same voxel, cap_leaves is too small. */
int64_t fluid_leaf_grids_merge(const fluid_leaf_grid_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin, float* values);

/* ---- liquid surface: narrow-band level set of the particles, as leaves (single GPU) ------------------------------------------
 * The density grid above is a one-cell blur of the particle set; this is the signed distance to the union of spheres of a fixed
 * radius around the particles, as OpenVDB's ParticlesToLevelSet::rasterizeSpheres leaves it (tools/ParticlesToLevelSet.h:591-643,
 * fixed radius; no prune, no renormalisation, Rmin not applied), restated as a function of the particle SET — a minimum, so no
 * particle order is involved.  All quantities in index space: voxel c is the integer point c, a particle's coordinates are the
 * handle's.
 *   R = (float)radius, w = (float)half_width, dxf = (float)params.dx; every operation below rounded to float:
 *   bg = dxf * w, mx = R + w, max2 = mx * mx, mn = max(0.0f, R - w), min2 = mn * mn.
 *   A live particle counts iff its base cell round(p) (half away from zero) lies in [lo,hi]^3.
 *   Squared distance of voxel c and particle P (differences and squares in double, narrowed to float after each axis, no FMA):
 *     x2 = (float)((cx - Px) * (cx - Px));  x2y2 = (float)((double)x2 + (cy - Py) * (cy - Py));
 *     x2y2z2 = (float)((double)x2y2 + (cz - Pz) * (cz - Pz))
 *   m = the minimum of x2y2z2 over the counted particles.  The voxel is inactive +bg if there is no particle or m >= max2;
 *   inactive -bg if m <= min2; otherwise d = dxf * (sqrtf(m) - R) (sqrtf correctly rounded): active with value d if d < bg, else
 *   inactive +bg.
 * Only voxels of [lo,hi]^3 are computed.  Leaves are OpenVDB's (origins at multiples of 8); a leaf is listed iff one of its in-grid
 * voxels is anything but inactive +bg; voxels of a listed leaf outside the grid are inactive +bg, as is every voxel of an unlisted
 * leaf.  The list is ascending in (x, y, z) origin.
 * Limits: radius > 0, half_width >= 1, R + w <= 4 (float sum), else FLUID_ERR_ARG: a particle within mx of a voxel then has its
 * base cell at Chebyshev distance <= 4 from it, so the search stays inside a 9^3 neighbourhood of cells.  A decomposed handle
 * returns FLUID_ERR_STATE from the three handle entry points below and takes its surface rank by rank with the next section
 * ("liquid surface (decomposed runs)").  Parity of the file with the library is unpinned
 * (as for the density files); the tests re-read it with their own reader. */
typedef struct fluid_sdf_params { double radius, half_width; } fluid_sdf_params_t;   /* voxels */
typedef struct fluid_sdf_grid {
    int32_t n, n_leaves;
    float background;            /* bg                                                                               */
    float radius, half_width;    /* R, w as used                                                                     */
    const int32_t* origin;       /* 3 per leaf                                                                       */
    const float* values;         /* 512 per leaf, ((x&7)*8 + (y&7))*8 + (z&7)                                        */
    const uint64_t* active;      /* 8 words per leaf: voxel off -> word off>>6, bit off&63 (OpenVDB NodeMask order)   */
} fluid_sdf_grid_t;
#define FLUID_SDF_LEAF_BYTES (2048 + 64 + 12)   /* a listed leaf on the way to the host: values, mask, origin            */
/* Captures the particles as they are at the call (after a step: after FLIPadvect and the sources / sinks; also right after an
 * upload).  Lifetime rules of the density snapshot above: kernels on the handle's stream, the 4-byte count of listed leaves read back,
 * the records copied to pinned host memory on a second stream and not waited for; two snapshots may be outstanding, a third returns
 * FLUID_ERR_STATE; buffers grow here, never inside a step, and are freed by the destroy call after the copies in flight have ended.
 * Before the kernels are sized the particles' base-cell box is read back as well (24 bytes; not part of bytes_to_host).
 * The slots and the count of outstanding snapshots are the surface's own: a caller can take this and a density snapshot per step.
 * Nothing a later step reads is written: the snapshot bins the particles into scratch of its own. */
int fluid_sdf_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p);
/* The oldest snapshot not yet waited for (FLUID_ERR_STATE when there is none); with no listed leaf n_leaves = 0 and the pointers
 * are NULL.  The pointers stay valid until the SECOND following surface snapshot on the handle. */
int fluid_sdf_wait(fluid_sim_t* s, fluid_sdf_grid_t* out);
/* Of the last snapshot (any pointer may be NULL): bytes_to_host = leaves_listed * FLUID_SDF_LEAF_BYTES + 4. */
int fluid_sdf_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host);
/* Host only: values[n^3] (z fastest) = +bg and active[n^3] (may be NULL) = 0 everywhere, then the in-grid voxels of every listed
 * leaf.  FLUID_ERR_ARG on an origin that is not a multiple of 8, lies outside the leaves of [lo,hi]^3 or is not strictly ascending. */
int fluid_sdf_to_dense(const fluid_sdf_grid_t* g, float* values, uint8_t* active);
/* Host only: one FloatGrid named "surface" (Tree_float_5_4_3, background bg, grid class "level set", file format 224) whose
 * topology is the listed leaves only — background tiles elsewhere — with the active masks as leaf value masks and the inactive
 * values coded by the per-node metadata byte of io/Compression.h.  Voxel size = background / half_width (float division: params.dx
 * whenever dxf * w is exact).  compression: FLUID_VDB_ACTIVE_MASK or FLUID_VDB_ZIP_ACTIVE_MASK.  Bad lists as above; an inactive
 * value that is neither +bg nor -bg is FLUID_ERR_ARG too, and so is a path that cannot be opened or written in full (the
 * partial file is removed). */
int fluid_write_vdb_sdf(const char* path, const fluid_sdf_grid_t* g, int32_t compression);

/* ---- liquid surface (decomposed runs) --------------------------------------------------------------------------------------
 * A voxel's value is a monotone function of the MINIMUM of x2y2z2 over the particles, and a minimum over a union of sets is the
 * minimum of the per-set minima: every rank takes the surface of its own particles, and a host merge joins the lists exactly.  No
 * ghost particles, no halo, no transport call; the rule is the same in decomposed and in replicated mode (both shard the particles).
 *
 * Rank-local list.  fluid_dist_sdf_snapshot on a decomposed handle gives exactly the list fluid_sdf_snapshot would give on a one-GPU
 * handle of the same N that holds this rank's LIVE particles and nothing else.  Live: the particles fluid_download_particles_ids
 * returns — after a step the arrays still hold the ghosts that were served and the particles a sink removed, marked dead and with
 * stale positions: they do not count.  The base cell must lie in [lo,hi]^3 as above.  Coordinates on a decomposed handle are global
 * index-space coordinates, so origins are global.  The list covers every leaf this rank's particles reach (their base-cell box dilated
 * by 4 cells, clipped to the grid), NOT the owned block: after FLIPadvect a rank's particles may sit outside its block, and a voxel
 * near a cut plane is reached from both sides.
 *
 * Merge.  The merged list is the union of the parts' leaves, ascending (x, y, z); a part that does not list a leaf contributes
 * inactive +bg in all of its voxels.  Per voxel, over the parts:
 *   1. some part holds it inactive with value -bg: the result is inactive -bg;
 *   2. otherwise, some part holds it active: active with the smallest active value (equal values: the first such part's bits);
 *   3. otherwise inactive +bg.
 * Exact: d = dxf * (sqrtf(m) - R) is a composition of correctly rounded monotone operations, so the smallest m gives the smallest d,
 * and m <= min2 on any part holds for the union too.  The three states are ordered by this rule, not by their float values: a plain
 * minimum of the values is not the merge.  For the lists the ranks of a run give, the merge is the list fluid_sdf_snapshot gives for
 * the union of their live particles.
 *
 *   per step, every rank:    fluid_step(s, &st);  fluid_dist_sdf_snapshot(s, &sp);  fluid_dist_sdf_wait(s, &part[rank]);
 *   one place:               k = fluid_sdf_grids_merge(part, R, cap, origin, values, active);
 *                            g = {n, k, bg, radius, half_width, origin, values, active};  fluid_write_vdb_sdf(path, &g, ...);
 * The particles survive a re-balancing of the cut planes (unlike the fields), so a snapshot the caller takes after fluid_step is exact
 * whether or not the step moved the planes: there is no `every` form.
 */
/* fluid_sdf_snapshot in every respect but the particles that count (above): kernels on the handle's stream, the 24-byte box and the
 * 4-byte count read back, the records copied on a second stream and not waited for, two snapshots may be outstanding (a third:
 * FLUID_ERR_STATE), buffers grow here and never inside a step.  A plain fluid_create handle is accepted: the list is
 * fluid_sdf_snapshot's, and both forms share the handle's two slots and its count of outstanding snapshots. */
int fluid_dist_sdf_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p);
/* The oldest snapshot not yet waited for, as fluid_sdf_wait; out->n is the global N; a rank with no counted particle gets
 * n_leaves = 0 and NULL pointers.  The pointers stay valid until the SECOND following surface snapshot on the handle — also across a
 * step that moves the cut planes (FLUID_PATH_DIST_REBALANCED). */
int fluid_dist_sdf_wait(fluid_sim_t* s, fluid_sdf_grid_t* out);
/* leaves_in_grid = the leaves of the GLOBAL grid, as fluid_sdf_stats; the other two of this handle's last snapshot:
 * bytes_to_host = leaves_listed * FLUID_SDF_LEAF_BYTES + 4.  Any pointer may be NULL. */
int fluid_dist_sdf_stats(fluid_sim_t* s, int64_t* leaves_in_grid, int64_t* leaves_listed, int64_t* bytes_to_host);
/* Host only.  The merge defined above into origin[3 * cap_leaves] / values[512 * cap_leaves] / active[8 * cap_leaves].  Returns the
 * merged leaf count (origin == values == active == NULL: the count only, cap_leaves is ignored), or -FLUID_ERR_ARG with nothing
 * written: n_parts < 1; the parts' n, background, radius or half_width differ as bit patterns; a part breaks the list rules of
 * fluid_sdf_to_dense; an inactive voxel of a part holds neither +bg nor -bg; cap_leaves is too small.  Parts with n_leaves == 0 and
 * NULL pointers are valid. */
int64_t fluid_sdf_grids_merge(const fluid_sdf_grid_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin, float* values,
                              uint64_t* active);

/* ---- liquid surface, smoothed: box filter and offset of the level set ------------------------------------------------------
 * The level set above is the raw union of spheres: a surface of bumps one particle wide.  OpenVDB pipelines put LevelSetFilter
 * between ParticlesToLevelSet and VolumeToMesh (mean or gaussian flow, then an offset that gives back the volume the flow took);
 * this is that stage, restated from the library's arithmetic (tools/LevelSetFilter.h:213-222, 231-233, 303-310, 471, 530-535) as
 * an exact, order-free definition of its own: the kernels, fluid_sdf_filter below and the tests' numpy form give the same bytes.
 *
 * Input.  The level set of "liquid surface": val(c) and act(c), c in [lo,hi]^3; every voxel of an unlisted leaf is inactive +bg,
 * and OUTSIDE THE GRID val is +bg (what the library's accessor returns outside the tree).  Float throughout, no FMA.
 *
 * One box pass of width W along axis a.  frac = 1.0f / (float)(2W + 1), one correctly rounded float division.  For every ACTIVE
 * voxel c:  s = 0.0f;  for i = -W .. +W ascending: s = s + val_prev(c + i e_a);  val_new(c) = s * frac.  Inactive voxels keep
 * their value (+bg or -bg).  val_prev is the complete result of the pass before (Jacobi, never in place); a voxel's sum has a
 * fixed order and depends on nothing but its inputs, so no schedule can change the result.
 * One iteration = three passes in the library's order: axis x, then axis Z, then axis Y (Filter::box binds boxX, boxY, boxZ in
 * that order, and boxY is Avg<2>).  After K iterations the offset: off = (float)offset; if off != 0.0f every active voxel gets
 * val = val + off (negative: the liquid grows); off == 0.0f skips the step, so K = 0 with offset 0 gives the unfiltered bytes.
 * Topology does not change: the active masks, the set of listed leaves and their order stay, inactive values stay +-bg, only
 * the values of active voxels differ.
 *
 * What this is not.  By itself the filter does NOT run LevelSetTracker::track() (the library's mean() / gaussian() run it after
 * every box): no renormalisation unless it is switched on — "liquid surface, renormalised" below — and never a rebuild (dilation)
 * of the band; mean(W) corresponds to K = 1, gaussian(W) to K = 4.  Untracked, an offset of more than about
 * bg - dx in magnitude pushes the surface into the band's edge, where the inactive +-bg plateau begins.
 * Limits: width in 1..4, iterations in 0..16, offset finite; anything else is FLUID_ERR_ARG.
 *
 * fluid_dist_sdf_snapshot stays unfiltered: a mean of per-rank minima is not the mean of the minimum.  A decomposed run filters
 * after the merge:  k = fluid_sdf_grids_merge(...);  g = {n, k, ...};  fluid_sdf_filter(&g, &f, smooth);  g.values = smooth;
 * then fluid_write_vdb_sdf / fluid_sdf_mesh as before. */
typedef struct fluid_sdf_filter { int32_t width; int32_t iterations; double offset; } fluid_sdf_filter_t;
/* fluid_sdf_snapshot in every respect (same two slots, same count of outstanding snapshots — the third is FLUID_ERR_STATE —, same
 * fluid_sdf_wait / fluid_sdf_stats), with 3 * iterations box passes (one more pass for an offset when iterations is 0) on the
 * handle's stream between the search and the pack.  The passes ping-pong between the search's values and a second buffer of the
 * same size, which the handle's first filtered snapshot allocates (never inside a step; an unfiltered caller never pays for it).
 * FLUID_ERR_ARG: bad parameters or bad filter limits.  FLUID_ERR_STATE on a decomposed handle: filter the merged list
 * (fluid_sdf_filter). */
int fluid_sdf_snapshot_filtered(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f);
/* fluid_mesh_snapshot ("liquid surface as a mesh", below) of the filtered level set: same slots, count, fluid_mesh_wait /
 * fluid_mesh_stats.  The front half runs over the particles' base-cell box dilated by 5 cells (unfiltered: 4): after the filter an
 * inside voxel is only known to be active or -bg, hence within R + w <= 4 of a particle and within 4 cells of its base cell, and the
 * min corner of a mixed cell lies in [-5, +4] of it.  Errors as above (FLUID_ERR_STATE names fluid_sdf_filter and fluid_sdf_mesh). */
int fluid_mesh_snapshot_filtered(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f);
/* Host only: the definition above applied to a leaf list; values[512 * n_leaves] receives the filtered values in the list's order
 * (g's own arrays are only read).  Voxels of listed leaves outside the grid are read as +bg and copied unchanged.  Works leaf by
 * leaf, the two neighbours on the pass's axis found by bisection; no dense grid is made.  FLUID_ERR_ARG with nothing written: a
 * list fluid_sdf_to_dense refuses, bad filter limits, values NULL with leaves, values overlapping g->values. */
int fluid_sdf_filter(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, float* values);

/* ---- liquid surface, renormalised: normalise and trim after every filter step ---------------------------------------------------
 * A box pass flattens the field: after it |grad val| is no longer 1, the values are no signed distance, `val + offset` moves the
 * surface by `offset` only where the slope is 1, and every later iteration smooths a flatter field than the library would.
 * LevelSetFilter therefore runs LevelSetTracker::track() after every box iteration and after every offset step.  This is that
 * stage — normalize() with the FIRST_BIAS / TVD_RK1 scheme, then Trim — restated from the library's arithmetic
 * (tools/LevelSetTracker.h:293-306, 455-475, 485-494, 596-609; math/Operators.h:252-284; math/FiniteDifference.h:352-374;
 * math/Math.h:118; the offset's steps: tools/LevelSetFilter.h:352-368) as an exact, order-free definition of its own: the kernel,
 * fluid_sdf_filter_tracked below and the tests' numpy form give the same bytes.
 *
 * Constants: dx = (float)params.dx, dt = dx * 0.3f, inv = 1.0f / dx, tol = 1e-8f, bg = the level set's background.  Float
 * throughout, no FMA, IEEE division and square root, denormals kept.  max(a, b) is a < b ? b : a and min(a, b) is b < a ? b : a.
 * Input: val, act as in "liquid surface, smoothed": unlisted leaves and everything outside the grid read as +bg, inactive voxels
 * as their stored +-bg.
 *
 * One normalisation pass (Jacobi: it reads only the complete result of the pass before).  Every ACTIVE voxel c, p = val(c):
 *   out = p > 0;  per axis a in the order x, y, z:  dm = p - val(c - e_a), dp = val(c + e_a) - p,
 *     out:  A = max(dm, 0), B = min(dp, 0);   otherwise:  A = min(dm, 0), B = max(dp, 0);   t_a = max(A*A, B*B);
 *   G = t_x;  G = G + t_y;  G = G + t_z;   S = p / (sqrtf(p*p + G) + tol);   val_new(c) = p - (dt * S) * (sqrtf(G) * inv - 1.0f).
 * Inactive voxels keep their value.
 * Trim.  An active voxel with val <= -bg becomes inactive -bg, one with val >= bg inactive +bg.
 * track(N, trim) = N normalisation passes, then the trim if `trim`.
 *
 * With tracking on (N > 0 or trim), a filter (W, K, offset) is: K times the three box passes x, z, y and then one track; then the
 * offset in the library's steps:  off = (float)offset, CFL = 0.5f * dx, a = fabsf(off), d = 0.0f;  while a - d > 0.001f * CFL:
 * delta = (a - d < CFL) ? a - d : CFL;  d = d + delta;  every active voxel gets val + copysignf(delta, off);  then one track.
 * fabsf(off) > bg is FLUID_ERR_ARG (no surface would be left; it also bounds the launches).  K = 0 with off == 0 runs nothing.
 * Tracking off, or N = 0 with trim = 0, is "liquid surface, smoothed" byte for byte, its single-step offset included.
 *
 * What holds.  Where G * inv^2 >= 1 the correction is smaller than 0.3 |p| in magnitude and directed towards 0; where it is < 1
 * the correction moves p away from 0; for p = 0, S = 0.  So a normalisation pass never changes a voxel's sign (up to rounding),
 * and the trim keeps the sign class: with K = 1 and no offset the mesh of the tracked level set has the untracked mesh's vertex
 * and quad COUNTS, only positions move, and the range argument of fluid_mesh_snapshot_filtered (the particles' box dilated by 5)
 * holds unchanged for the tracked mesh and image.
 * Listing.  A leaf is listed iff it holds anything but inactive +bg, evaluated AFTER the last trim: trimming can unlist leaves and
 * can empty the list (n_leaves = 0).  Attributes: a voxel the trim deactivated has FLUID_SDF_NO_ID and +0 velocity like every
 * other inactive voxel; ids and velocities of the voxels still active are untouched.
 *
 * What this is not.  By itself the band never grows: dilateActiveValues, the first line of track(), is run only with growing
 * switched on ("liquid surface, grown band" below); without it a surface that leaves the band is lost to the trim instead of
 * followed.  The library's default spatial scheme, HJWENO5, is the scheme FLUID_SDF_TRACK_HJWENO5 ("liquid surface, renormalised:
 * HJWENO5" below); the other spatial schemes (SECOND_BIAS, THIRD_BIAS, WENO5_BIAS) and TVD_RK2/3 are not built; neither are the
 * tracker's dilate / erode / resize.  Decomposed handles take no tracked snapshots: track the merged list. */
#define FLUID_SDF_TRACK_FIRST_BIAS 0   /* the library's own BiasedGradientScheme numbers (math/FiniteDifference.h:192-199) */
#define FLUID_SDF_TRACK_HJWENO5 4      /* "liquid surface, renormalised: HJWENO5" below; 1, 2, 3 and everything else: FLUID_ERR_ARG */
typedef struct fluid_sdf_track { int32_t normalize; /* passes per track: 0..8; the library's default is 3 */
                                 int32_t trim;      /* 0 or 1 */
                                 int32_t scheme;    /* FLUID_SDF_TRACK_FIRST_BIAS or FLUID_SDF_TRACK_HJWENO5 */ } fluid_sdf_track_t;
/* A setting of the handle, like fluid_set_dt: every later snapshot that is given a filter runs the tracked form of it —
 * fluid_sdf_snapshot_filtered, fluid_sdf_snapshot_attr, fluid_mesh_snapshot_filtered, fluid_mesh_snapshot_attr,
 * fluid_mesh_snapshot_ex and fluid_render_snapshot; unfiltered snapshots are untouched.  NULL: off (the default).  One launch per
 * normalisation pass on the handle's stream, one more after the last trim; the scratch it needs is allocated by the first tracked
 * snapshot, never inside a step.  FLUID_ERR_ARG: bad limits or an unknown scheme.  FLUID_ERR_STATE on a decomposed handle: track
 * the merged list (fluid_sdf_filter_tracked). */
int fluid_sdf_set_track(fluid_sim_t* s, const fluid_sdf_track_t* t);
/* Host only: the tracked filter applied to a leaf list, how a block run gets it after fluid_sdf_grids_merge.  Returns the number
 * of leaves still listed and writes the compacted list: origin[3 k] ascending, values[512 k], active[8 k], and, when kept is not
 * NULL, kept[i] = the index in g of output leaf i (to gather attribute arrays by).  With origin, values and active all NULL it
 * returns the count only.  t == NULL (and N = 0 with trim = 0): fluid_sdf_filter plus the copy of masks and origins; every leaf
 * stays.  dx is background / half_width (a list carries no dx), or the float next to that quotient whose product with half_width
 * gives the background back.  Voxels of listed leaves outside the grid are read as +bg, copied unchanged, and do not count for the listing.  Works
 * leaf by leaf, the six face neighbours found by bisection; no dense grid is made.  -FLUID_ERR_ARG with nothing written: whatever
 * fluid_sdf_filter refuses, bad track limits, fabsf(offset) > background with tracking on, cap_leaves smaller than the count,
 * some but not all of the three outputs NULL, outputs overlapping g's arrays. */
int64_t fluid_sdf_filter_tracked(const fluid_sdf_grid_t* g, const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t,
                                 int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active, int32_t* kept /* may be NULL */);

/* ---- liquid surface, renormalised: HJWENO5 -------------------------------------------------------------------------------------------
 * The library's tracker defaults to HJWENO5_BIAS with TVD_RK1 (tools/LevelSetTracker.h:83-86); FIRST_BIAS above is what it runs
 * only when asked.  The first-order Godunov step is diffusive on curved surfaces: it moves an EXACT signed distance of a sphere of
 * radius 4 to 9 voxels by 0.05 to 0.1 voxel per track, HJWENO5 by about a thousandth (profiles/track/NOTES.md), so "an offset moves
 * the surface by the offset" holds only to that accuracy under FIRST_BIAS.  With scheme = FLUID_SDF_TRACK_HJWENO5 every
 * normalisation pass of every track forms its gradient term from seven values per axis.  Nothing else changes: the same launches
 * per pass, the same two value buffers, the same trim, dilation, offset steps, listing and attributes, the schedule of
 * sdf_filter_plan.h.  Restated from the library's arithmetic (tools/LevelSetTracker.h:596-609; math/Operators.h:252-284;
 * math/FiniteDifference.h:331-349, 352-374, 1224-1233, 1428-1435) as an exact, order-free definition of its own: the kernel
 * (kernels_sdf_weno.hip), the host functions below and the tests' numpy form give the same bytes; the arithmetic is stated once
 * for both compilers in csrc/sdf_weno_def.h.  Where this text and the cited lines differ the lines win.
 *
 * Only the gradient term of "liquid surface, renormalised" changes.  For an ACTIVE voxel c with p = val(c), and per axis a in the
 * order x, y, z, let u(k) = val(c + k e_a) for k = -3..3.  Reads follow the rule above: unlisted leaves and everything outside the
 * grid read +bg, inactive voxels their stored +-bg.  All differences are float subtractions.
 *   dp =  W5(u(3)-u(2),   u(2)-u(1),   u(1)-u(0),  u(0)-u(-1), u(-1)-u(-2))
 *   dm = -W5(u(-3)-u(-2), u(-2)-u(-1), u(-1)-u(0), u(0)-u(1),  u(1)-u(2))
 *   t_a from (out, dm, dp) exactly as above (A, B, max(A*A, B*B)); G, S and val_new exactly as above.
 * W5(v1..v5) takes floats and returns a float; it works in double where the library's expression promotes (WENO5<float> with its
 * default scale2 = 0.01f).  sqf is a float product, sqd a double product:
 *   C = 13.0/12.0;  eps = 1.0e-6 * (double)0.01f
 *   s1 = (C*(double)sqf((v1 - 2.0f*v2) + v3) + 0.25*sqd((double)(v1 - 4.0f*v2) + 3.0*(double)v3)) + eps
 *   s2 = (C*(double)sqf((v2 - 2.0f*v3) + v4) + 0.25*(double)sqf(v2 - v4)) + eps
 *   s3 = (C*(double)sqf((v3 - 2.0f*v4) + v5) + 0.25*sqd((3.0*(double)v3 - (double)(4.0f*v4)) + (double)v5)) + eps
 *   A1 = 0.1/(s1*s1);  A2 = 0.6/(s2*s2);  A3 = 0.3/(s3*s3)
 *   num = (A1*((2.0*v1 - 7.0*v2) + 11.0*v3) + A2*((5.0*v3 - v2) + 2.0*v4)) + A3*((2.0*v3 + 5.0*v4) - v5)      (double)
 *   W5  = (float)( (double)(float)num / (6.0*((A1 + A2) + A3)) )
 * No FMA, in float or in double; IEEE division and square root, in float and in double; denormals kept.
 *
 * What still holds.
 * Signs: G >= 0 whatever formed it, and the step is the one above, so where sqrtf(G) * inv >= 1 the correction is at most 0.3 |p|
 * and directed towards 0, elsewhere it moves p away from 0, and p = 0 gives S = 0: a pass changes no sign (up to rounding).  With
 * K = 1 and no offset the mesh of the tracked level set has the untracked mesh's vertex and quad counts.
 * Finite: eps > 0 keeps s1, s2, s3 positive, so A1, A2, A3 and their sum are positive and finite for finite input, and G is finite.
 * Range: a stencil of depth 3 along the axes still needs face neighbours only (a leaf is 8 deep), and everything outside the
 * device's range of leaves is inactive +bg in truth, so the ranges of "grown band" (4 + T, 5 + T for the mesh and the image) and
 * of fluid_mesh_snapshot_filtered need no change.
 * Symmetries of the definition (checked on the reference, tests/test_sdf_weno_ref.py): negating the seven values negates dm and dp
 * bit for bit; reversing them gives (-dp, -dm) bit for bit.
 *
 * Where it applies.  fluid_sdf_set_track takes the scheme, and with it every entry point that takes a filter on a one-GPU handle
 * (the list at fluid_sdf_set_track), grown tracks and every filter kind included.  On the host fluid_sdf_filter_tracked,
 * fluid_sdf_filter_grown and fluid_sdf_flow run the scheme their fluid_sdf_track_t names, the six face neighbours read three
 * planes deep.  Schemes 1, 2, 3, anything >= 5 and negatives stay FLUID_ERR_ARG; decomposed handles stay FLUID_ERR_STATE.
 *
 * What this is not.  TVD_RK2 / TVD_RK3 (they need a third buffer); SECOND_BIAS, THIRD_BIAS, WENO5_BIAS; fused passes.  Parity of the
 * results with the library's own output is unpinned, as for the other surface sections: the definition is restated from its source. */

/* ---- liquid surface, grown band: dilate, normalise, trim ---------------------------------------------------------------------------
 * "Liquid surface, renormalised" stops one line short of the library's track(), which is dilateActiveValues(leafs, 1, NN_FACE, IGNORE_TILES),
 * normalize(), prune() (tools/LevelSetTracker.h:299, 302, 305).  Without the dilation the band stays where the rasteriser put it:
 * a tracked offset cannot exceed bg, and within bg the surface runs into the rim of a band that does not follow it.  With growing
 * on every track begins with one dilation, so the band walks with the surface — outwards through +bg, inwards through the
 * inactive -bg interior.  An exact, order-free definition: the kernel (kernels_sdf_grow.hip), fluid_sdf_filter_grown below and
 * the tests' numpy form give the same bytes.
 *
 * One dilation.  Input val, act as in "liquid surface, smoothed".  For every voxel c of [lo,hi]^3:
 *   act_new(c) = act(c) OR act of any of its six face neighbours; a neighbour outside the grid is inactive.
 * Values do not change: a newly active voxel keeps its stored inactive value, -bg or +bg (+bg is what every voxel of an unlisted
 * leaf holds).  Voxels of a leaf outside the grid never become active.  Jacobi: the masks are read as they were before the
 * dilation.  The dilation is clipped by the grid and by nothing else — no range of an implementation clips it.
 * Grown track = one dilation, then N normalisation passes, then the trim (tdef::track_value, tdef::trim_class, unchanged).
 *
 * Settings and limits.  Growing requires normalize >= 1 and trim = 1: that is the library's track().  A filtered snapshot taken
 * with growing on and any other track setting, or with tracking off, is FLUID_ERR_ARG.
 * Tracked filter with growing on = "liquid surface, renormalised" with every track replaced by the grown track: the box
 * iterations, the stepped offset and tdef::offset_step stay; the offset limit becomes fabsf(off) > 4.0f * dx -> FLUID_ERR_ARG
 * (instead of > bg); a leaf is listed iff it holds anything but inactive +bg after the last trim, and the list can now hold leaves
 * the unfiltered list does not.  K = 0 with off == 0 runs nothing.
 *
 * Attributes (an extension of this project's own: the library does not extend its attribute grid).  A voxel that a dilation
 * activates takes the id and velocity of the first of its face neighbours, in the order -x, +x, -y, +y, -z, +z, that was active
 * BEFORE that dilation.  That neighbour carries an id, by induction: initially active voxels have one, the trim gives
 * FLUID_SDF_NO_ID only to voxels it deactivates, and a voxel activated later inherits again.  So "active <=> id != FLUID_SDF_NO_ID"
 * still holds and the vertex-velocity rule of "liquid surface, attributes" needs no change.
 *
 * Range.  After T grown tracks the active set lies within the Manhattan dilation by T of the initial one, which lies within 4
 * cells (Chebyshev) of the particles' base-cell box.  T = iterations + the number of offset steps is known on the host before
 * anything is sized, so the device works on the leaves of that box dilated by 4 + T cells — 5 + T for the mesh and the image, by
 * the argument at fluid_mesh_snapshot_filtered: an inside voxel is active or inactive -bg, hence within 4 + T cells of the box
 * (the trim makes -bg only of active voxels), and a mixed cell's min corner is one cell below an inside voxel at most — clipped
 * to the grid: exact, no clipping by the range ever happens.  The scratch for the larger range is allocated by the snapshot call, never inside a step, and only a
 * handle that has taken a grown snapshot pays for it.
 * With growing off every byte of every entry point is what it was.
 *
 * What this is not.  LevelSetTracker::dilate(n) / erode / resize, which change the half width and the background; tracked
 * rank snapshots of decomposed handles; a two-offset "closing" entry point — a caller composes one on the host with two
 * fluid_sdf_filter_grown calls. */
/* A setting of the handle like fluid_sdf_set_track, and independent of it in order: grow = 1 makes every later filtered snapshot
 * (the list of fluid_sdf_set_track) run grown tracks; 0 (the default): off.  The rule "normalize >= 1 and trim = 1" is checked
 * where a filtered snapshot begins: FLUID_ERR_ARG from that snapshot; unfiltered snapshots are untouched.  One more launch per
 * track; a second set of masks and flags, which the launch writes while it reads the first (no block reads a word another block
 * of the launch writes), is allocated by the first grown snapshot.  FLUID_ERR_ARG: grow is neither 0 nor 1.  FLUID_ERR_STATE on a
 * decomposed handle: grow the merged list (fluid_sdf_filter_grown). */
int fluid_sdf_set_track_grow(fluid_sim_t* s, int32_t grow);
/* Host only: the grown filter applied to a leaf list, how a block run gets it after fluid_sdf_grids_merge /
 * fluid_sdf_attr_grids_merge.  Returns the number of leaves listed and writes the new list, which can be longer than g's:
 * origin[3 k] ascending, values[512 k], active[8 k], and with attr (ids and velocities of g's leaves, attr->n_leaves ==
 * g->n_leaves) id[512 k] and velocity[3 * 512 k] in full — there is no `kept`: grown leaves have no source leaf.  A leaf the
 * dilation adds holds +bg, FLUID_SDF_NO_ID and +0 wherever nothing was activated, its voxels outside the grid included.  With all
 * five outputs NULL it returns the count only.  dx, the voxels of listed leaves outside the grid (never active, never a
 * neighbour, copied unchanged) and the listing are fluid_sdf_filter_tracked's.  Works leaf by leaf on a working copy of the list,
 * the six face neighbours found by bisection; no dense grid is made.  -FLUID_ERR_ARG with nothing written: whatever
 * fluid_sdf_filter refuses; t NULL, normalize outside 1..8, trim != 1 or an unknown scheme; fabsf(offset) > 4 dx; attr whose
 * n_leaves differs or whose arrays are NULL with leaves; id or velocity NULL with attr, or given without it; cap_leaves smaller than
 * the count; some but not all of origin, values and active NULL; outputs overlapping g's or attr's arrays. */
struct fluid_sdf_attr;   /* fluid_sdf_attr_t: "liquid surface, attributes" below */
int64_t fluid_sdf_filter_grown(const fluid_sdf_grid_t* g, const struct fluid_sdf_attr* attr /* may be NULL */, const fluid_sdf_filter_t* f,
                               const fluid_sdf_track_t* t, int64_t cap_leaves, int32_t* origin, float* values, uint64_t* active,
                               uint32_t* id /* NULL iff attr NULL */, float* velocity /* likewise */);

/* ---- liquid surface, flows: median, Laplacian and mean-curvature flow of the level set --------------------------------------------
 * The three other filters of the library's LevelSetFilter.  The box filter blurs: it rounds off thin sheets as fast as it removes
 * the one-particle bumps of the sphere union.  median(width) removes the bumps and keeps edges, meanCurvature() is the standard
 * fairing step before meshing, and laplacian() is its cheap equivalent once the field is renormalised (the library says so itself,
 * tools/LevelSetFilter.h:411-417).  Restated from the library's arithmetic (tools/LevelSetFilter.h:256-268, 318-347, 380-409,
 * 421-450, 481-507; math/Stencils.h:147-155, 1230-1238, 1283-1288, 1506-1540, 1596-1619, 1670-1680; math/Math.h:119) as an exact,
 * order-free definition of its own: the kernels (kernels_sdf_flow.hip), fluid_sdf_flow below and the tests' numpy form give the
 * same bytes; the arithmetic is stated once for both compilers in csrc/sdf_flow_def.h.
 *
 * Common rules.  Input val, act as in "liquid surface, smoothed": unlisted leaves and everything outside the grid read as +bg,
 * inactive voxels as their stored +-bg.  Each pass is Jacobi (it reads only the complete result of the pass before).  Only ACTIVE
 * voxels get a new value; topology does not change, inactive voxels keep their value, attributes are untouched.
 * dx = (float)params.dx.  No FMA anywhere; IEEE division and square root, float and double.  Neighbours: xm = val(c - e_x),
 * xp = val(c + e_x), likewise y and z; v(i,j,k) = val(c + (i,j,k)); p = val(c).
 * Shared constants: inv2dx = (float)(0.5 / (double)dx);  invdx2 = (float)(4.0 * (double)inv2dx * (double)inv2dx).
 *
 * Laplacian (GradStencil).  All float.  dt = (dx * dx) / 6.0f;
 *   L = invdx2 * ((((((xm + xp) + ym) + yp) + zm) + zp) - 6.0f * p);   val_new = p + dt * L.
 *
 * Mean curvature (CurvatureStencil::meanCurvatureNormGrad).  Differences are taken in FLOAT and then widened; everything after
 * that is DOUBLE (the library's Real), and the term is narrowed once.  dt = (dx * dx) / 3.0f;
 *   Dx = 0.5 * (double)(xp - xm), Dy, Dz likewise;  Dx2 = Dx * Dx, Dy2, Dz2 likewise;  ng = (Dx2 + Dy2) + Dz2.
 *   ng <= 1e-15 (math::Tolerance<double>):  F = 0.0f.  Otherwise:
 *   Dxx = (double)((xp - 2.0f * p) + xm), Dyy, Dzz likewise;
 *   Dxy = 0.25 * (double)(((v(1,1,0) - v(1,-1,0)) + v(-1,-1,0)) - v(-1,1,0));
 *   Dxz = 0.25 * (double)(((v(1,0,1) - v(1,0,-1)) + v(-1,0,-1)) - v(-1,0,1));
 *   Dyz = 0.25 * (double)(((v(0,1,1) - v(0,1,-1)) + v(0,-1,-1)) - v(0,-1,1));
 *   alpha = ((Dx2*(Dyy+Dzz) + Dy2*(Dxx+Dzz)) + Dz2*(Dxx+Dyy)) - 2.0*((Dx*((Dy*Dxy) + (Dz*Dxz))) + ((Dy*Dz)*Dyz));
 *   beta = sqrt(ng);   F = (float)((alpha * (double)invdx2) / (2.0 * (beta * beta)));
 *   val_new = p + dt * F in float.
 * 19 points: the centre, the six faces and the twelve edges; no corners.
 *
 * Median (DenseStencil, width W).  Take the m = (2W+1)^3 values of the cube around c; val_new is the element at zero-based rank
 * (m - 1) >> 1 in the order of the usual monotone 32-bit key: all bits of a negative float flipped, the sign bit of the others
 * set.  Under it -0 sorts before +0 and equal keys are equal bytes, so the result is a function of the multiset alone and any
 * selection method gives the same bytes.  Where this differs from the source: the library selects with std::nth_element under
 * operator<, for which -0 and +0 are equivalent, so which of the two zeros it returns at the median rank is its implementation's
 * choice; the key order decides it.  Values are always finite — the rasteriser's values lie in [-bg, bg], a box, Laplacian or
 * curvature pass and the track's step are finite arithmetic on at most 16 iterations of bounded growth, an offset is finite, and
 * the median returns one of its inputs — so no NaN ever reaches the key, whose order is total on everything else.
 *
 * Schedule.  One iteration of these three kinds is ONE pass (the box filter has three).  With tracking on each pass is followed by
 * one track, as the library does (LevelSetFilter.h:256-268, 318-347), grown if growing is on.  After the iterations the offset,
 * exactly as for the box filter: stepped under tracking, a single val + off otherwise.  T, the number of tracks, stays iterations
 * + offset steps.  A flow changes only active voxels, so the range argument for the mesh and the image is unchanged: the
 * particles' box dilated by 5, or by 5 + T when grown.
 * Limits.  Median: width 1 or 2 (the 27- and 125-value cubes; the library's default is 1, and its own comment calls the filter
 * "simple but slow").  Laplacian and mean curvature: width must be 1.  Iterations 0..16; the offset rules stay as they are.
 *
 * What this is not.  The alpha masks of the library's filters and Filter::fill are not built.  Parity of the results
 * with the library's own output is unpinned: the definitions are restated from its source. */
#define FLUID_SDF_FILTER_BOX 0
#define FLUID_SDF_FILTER_MEDIAN 1
#define FLUID_SDF_FILTER_LAPLACIAN 2
#define FLUID_SDF_FILTER_MEAN_CURVATURE 3
/* A setting of the handle beside fluid_sdf_set_track and fluid_sdf_set_track_grow, and independent of them in order: every later
 * snapshot that is given a filter — fluid_sdf_snapshot_filtered, fluid_sdf_snapshot_attr, fluid_mesh_snapshot_filtered,
 * fluid_mesh_snapshot_attr, fluid_mesh_snapshot_ex and fluid_render_snapshot — runs the passes of that kind in place of the box
 * passes.  The default is FLUID_SDF_FILTER_BOX, with which every byte of every entry point is what it was.  The width rule of the
 * kind is checked where a filtered snapshot begins: FLUID_ERR_ARG from that snapshot.  One launch per pass; no scratch beyond the
 * second value buffer of the filtered snapshots.  FLUID_ERR_ARG: an unknown kind.  FLUID_ERR_STATE on a decomposed handle: filter
 * the merged list (fluid_sdf_flow). */
int fluid_sdf_set_filter_kind(fluid_sim_t* s, int32_t kind);
/* Host only: the filter of `kind` applied to a leaf list, how a block run gets the flows after fluid_sdf_grids_merge /
 * fluid_sdf_attr_grids_merge.  t == NULL (and N = 0 with trim = 0): untracked, every leaf stays; t with grow = 0: the tracked
 * filter; grow = 1: the grown filter.  Outputs, the count-only call, dx from background / half_width, the voxels of listed leaves
 * outside the grid and the refusals follow fluid_sdf_filter_grown (the offset limit of the form that runs: none untracked, the
 * background tracked, 4 dx grown; a background and a half width are required where dx is read: tracked, or a Laplacian or
 * curvature pass), and beside them: an unknown kind, a width the kind does not admit, grow neither 0 nor 1.  With
 * kind = FLUID_SDF_FILTER_BOX it returns the bytes of fluid_sdf_filter, fluid_sdf_filter_tracked or fluid_sdf_filter_grown for
 * the same arguments.  Works leaf by leaf, the 26 neighbours found by bisection; no dense grid is made. */
int64_t fluid_sdf_flow(const fluid_sdf_grid_t* g, const struct fluid_sdf_attr* attr /* may be NULL */, int32_t kind,
                       const fluid_sdf_filter_t* f, const fluid_sdf_track_t* t /* NULL: untracked */, int32_t grow, int64_t cap_leaves,
                       int32_t* origin, float* values, uint64_t* active, uint32_t* id /* NULL iff attr NULL */,
                       float* velocity /* likewise */);

/* ---- liquid surface, averaged positions: the distance to a weighted average of the nearby particles -------------------------------
 * Every section above works on the bumps of the union of spheres after they are made; this one does not make them.  It is the
 * surface FLIP users know from Zhu and Bridson (the distance to a kernel-weighted average of the nearby particle positions: flat
 * over a flat pool), which OpenVDB does not have: a definition of the project's own, in the style of "liquid surface".  Unchanged
 * from there: the constants R, w, dxf, bg, max2, min2, which particles count, x2y2z2 (x2 below) exactly as stated there, m = the
 * minimum of x2 over the counted particles, and the leaf and list rules.  New, with hf = (float)influence:
 *   h2 = hf * hf, ih2 = 1.0f / h2 (float, the division correctly rounded).
 *   Weight of particle P at voxel c: W = 0 unless x2 < h2; otherwise t = 1.0f - x2 * ih2, wt = (t * t) * t (float, no FMA) and
 *     W = (int64)rintf(wt * 16777216.0f) — the product is exact, the rounding half to even, and W may be 0.
 *   Offset: O_a = (int64)rint((P_a - (double)c_a) * 262144.0) per axis a: one double subtraction, an exact scaling; |O_a| < 2^20.
 *   Sums over the counted particles: SW = sum of W, SX = sum of W * O_x, SY, SZ likewise: 64-bit integers added with wrap-around
 *     (unsigned arithmetic).  They are exact while fewer than 2^19 particles lie within hf of one voxel: that is the limit, and it
 *     is not checked.
 *   Averaged distance (SW > 0 only): den = (double)SW * 262144.0; ax = (double)SX / den, ay, az likewise (double divisions);
 *     a2 = (float)(ax * ax); a2 = (float)((double)a2 + ay * ay); a2 = (float)((double)a2 + az * az); da = dxf * (sqrtf(a2) - R).
 *   The voxel: no particle or m >= max2: inactive +bg.  m <= min2: inactive -bg.  Otherwise ds = dxf * (sqrtf(m) - R),
 *     d = SW > 0 ? fmaxf(da, ds) : ds; active with value d if d < bg, else inactive +bg.
 * The maximum with the spheres' distance is what keeps air gaps narrower than 2 hf open (the plain average fills them), and it
 * leaves a lone droplet a sphere.  Three things follow:
 *   d >= ds everywhere: the averaged liquid lies inside the union of spheres, its active set is a subset of the spheres' active set
 *     and its listed leaves a subset of theirs, so every range argument downstream (4 or 5 cells of dilation, growth) holds as it is.
 *   A particle whose base cell is k + 1 cells away has x2 >= (k + 0.5)^2 as computed (the ring argument of kernels_sdf.hip), so its
 *     weight is exactly 0 once (k + 0.5)^2 >= h2: with hf <= 4, ring 4 is the last.
 *   The sums need EVERY ring up to that one; m has earlier stops of its own, or simply rides along.
 * A value is a function of integer sums and a minimum over the particle set: order-free and bit-reproducible.
 * Limits: 0 < hf <= 4, else FLUID_ERR_ARG.  With hf < R + w the band voxels further than hf from every particle keep the spheres'
 * value (SW == 0): that is legal.
 * Decomposed runs: a rank record carries m and the four sums, and the merge is a minimum and integer additions, which is exact:
 * "liquid surface, averaged positions (decomposed runs)" below.  Attributes and anisotropic kernels are not built; radii per particle are those of
 * "liquid surface, velocity trails" below, a surface of its own. */
#define FLUID_SDF_SURFACE_SPHERES  0
#define FLUID_SDF_SURFACE_AVERAGED 1
typedef struct fluid_sdf_surface { int32_t kind; int32_t reserved; double influence; /* voxels; read with AVERAGED only */ } fluid_sdf_surface_t;
/* A setting of the handle beside fluid_sdf_set_track, fluid_sdf_set_track_grow and fluid_sdf_set_filter_kind, and independent of
 * them in order: every later fluid_sdf_snapshot, fluid_sdf_snapshot_filtered, fluid_mesh_snapshot, fluid_mesh_snapshot_filtered,
 * fluid_mesh_snapshot_ex (without FLUID_MESH_VELOCITY) and fluid_render_snapshot takes the level set defined above in place of the
 * spheres'; filters, tracks, growth, meshes and images work on it as they work on the spheres'.  NULL or kind
 * FLUID_SDF_SURFACE_SPHERES (the default): the spheres, every byte of every entry point what it was.  Under AVERAGED the attribute
 * entry points (fluid_sdf_snapshot_attr, fluid_mesh_snapshot_attr, FLUID_MESH_VELOCITY) and fluid_dist_sdf_snapshot /
 * fluid_dist_sdf_snapshot_attr (also on a plain handle) return FLUID_ERR_STATE.  FLUID_ERR_ARG: a kind other than the two, or
 * under AVERAGED reserved != 0 or an influence outside (0, 4].  FLUID_ERR_STATE on a decomposed handle, whose rank record takes the
 * surface as an argument instead (fluid_dist_sdf_snapshot_avg). */
int fluid_sdf_set_surface(fluid_sim_t* s, const fluid_sdf_surface_t* sf);
/* Host only, no handle: the dense level set of np particles (pos: x, y, z per particle, index-space coordinates) on the grid of
 * n^3 voxels of size dx, for either kind (sf NULL or SPHERES: "liquid surface"), brute force over the base cells within 4 of each
 * voxel: values[n^3] and active[n^3] (z fastest; active may be NULL).  The limits of p and sf are those of fluid_sdf_snapshot and
 * fluid_sdf_set_surface; n >= 1, dx > 0 and non-NULL pos (np > 0), p, values are required: FLUID_ERR_ARG.  It is how the definition
 * above is checked where there is no device, and what the search on the device is pinned to bit for bit. */
int fluid_particles_surface(int32_t n, double dx, int64_t np, const double* pos, const fluid_sdf_params_t* p, const fluid_sdf_surface_t* sf,
                            float* values, uint8_t* active);

/* ---- liquid surface, averaged positions (decomposed runs) --------------------------------------------------------------------------
 * Everything not restated here is that of "liquid surface" and "liquid surface, averaged positions".  A voxel of the averaged surface
 * is a function of a minimum and of four wrapping 64-bit integer sums over the particle set, and both split exactly over a partition
 * of the set: every rank records (m, SW, SX, SY, SZ) of its own live particles, and a host merge finishes the voxels.  No ghost
 * particles, no halo, no transport call.  Let reach2 = max(max2, h2) in float.
 *
 * Which leaves a rank lists.  The spheres' list is not enough: with hf > R + w a particle weighs on voxels outside its own band, and
 * such a voxel may lie inside the band of another rank's particle while this rank lists nothing there.  A rank lists a leaf iff
 * some in-grid voxel of it has m < reach2, m taken over this rank's live particles.
 *
 * What a rank stores per voxel of a listed leaf:
 *   min2 < m < reach2:                                            dist2 = m; SW, SX, SY, SZ over this rank's live particles
 *   m <= min2:                                                    dist2 = +0.0f; the four sums 0
 *   m >= reach2, no particle, or the voxel outside [lo,hi]^3:     dist2 = +inf (0x7f800000); the four sums 0
 * A voxel with m <= min2 on any rank is inactive -bg in every union, whatever the sums: that is why the record (and the search's
 * early stop of a plane, which leaves m and the sums of such voxels unfinished) may drop them.  The record is canonical: a function
 * of the rank's live particle set alone.  m is exact whenever m < reach2 (the ring argument above: a particle beyond the last ring
 * has x2 >= reach2).
 *
 * Merge, per voxel over the parts that list its leaf: m = the minimum of the parts' dist2 (+inf if none lists it); the sums = the
 * wrapping 64-bit sums of the parts' sums; the voxel = the rule of "liquid surface, averaged positions" applied to (m, sums).  A part
 * whose dist2 is +inf adds zero sums, rightly: its particles are further than hf.  Where some part holds +0 the result is inactive
 * -bg and the sums are not read.  The merged list holds the leaves with anything but inactive +bg, ascending, under the rules of
 * fluid_sdf_to_dense.  For the records the ranks of a run give, the result is byte for byte the list fluid_sdf_snapshot gives under
 * AVERAGED on one handle that holds the union of their live particles.
 *
 *   per step, every rank:    fluid_step(s, &st);  fluid_dist_sdf_snapshot_avg(s, &sp, &sf);  fluid_dist_sdf_wait_avg(s, &part[rank]);
 *   one place:               k = fluid_sdf_avg_grids_merge(part, R, cap, origin, values, active);
 *                            g = {n, k, bg, radius, half_width, origin, values, active};  filter / mesh / render / write as on one GPU.
 * The rank record is unfiltered and carries no attributes: a block run filters after the merge. */
#define FLUID_SDF_AVG_PART_LEAF_BYTES (2048 + 4 * 4096 + 12)   /* a listed leaf of a rank record on the way to the host */
typedef struct fluid_sdf_avg_part {
    int32_t n, n_leaves;
    float background, radius, half_width, dx, influence;   /* dx = (float)dx of the handle, influence = hf */
    const int32_t* origin;      /* 3 per leaf, ascending */
    const float* dist2;         /* 512 per leaf */
    const uint64_t* sums;       /* [leaf][4][512]: SW, SX, SY, SZ */
} fluid_sdf_avg_part_t;
/* fluid_dist_sdf_snapshot in every respect (live particles only, global coordinates, no transport call, the surface's own two slots
 * and their shared count of outstanding snapshots, survival of a re-balance) but the record, and the surface comes with the call:
 * sf must be of kind AVERAGED within the limits of fluid_sdf_set_surface, else FLUID_ERR_ARG; the handle's own surface setting is
 * neither read nor changed.  A plain fluid_create handle is accepted.  The record is [n x 2048 B dist2 | n x 16384 B sums |
 * n x 12 B origins]; fluid_dist_sdf_stats reports bytes_to_host = leaves_listed * FLUID_SDF_AVG_PART_LEAF_BYTES + 4.  The extra
 * scratch (32 B per voxel of the range for the sums, 4 B for dist2) is allocated by the handle's first such snapshot, never inside
 * a step; a slot keeps room for the longest record it has held. */
int fluid_dist_sdf_snapshot_avg(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_surface_t* sf);
/* The oldest snapshot not yet waited for, which must be an averaged rank record: on one of another kind FLUID_ERR_STATE, and the
 * snapshot stays outstanding.  Likewise fluid_sdf_wait, fluid_sdf_wait_attr, fluid_dist_sdf_wait and fluid_dist_sdf_wait_attr on an
 * averaged rank record.  A rank with no counted particle gets n_leaves = 0 and NULL pointers.  Lifetime of the pointers: that of
 * fluid_dist_sdf_wait's. */
int fluid_dist_sdf_wait_avg(fluid_sim_t* s, fluid_sdf_avg_part_t* out);
/* Host only.  The merge defined above into origin[3 * cap_leaves] / values[512 * cap_leaves] / active[8 * cap_leaves].  Returns the
 * merged leaf count (all three outputs NULL: the count only, cap_leaves is ignored), or -FLUID_ERR_ARG with nothing written:
 * n_parts < 1; parts whose n, background, radius, half_width, dx or influence differ as bit patterns, or are not what a snapshot
 * gives (the limits of p and sf, background = dx * half_width); a part that breaks the list rules of fluid_sdf_to_dense; a part with
 * n_leaves > 0 and a NULL array; a dist2 that is NaN or negative (-0 included); a voxel whose dist2 is +0 or +inf while one of its
 * sums is not 0; cap_leaves too small.  Parts with n_leaves == 0 and NULL pointers are valid.  A k-way walk of the ascending lists;
 * no dense grid. */
int64_t fluid_sdf_avg_grids_merge(const fluid_sdf_avg_part_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin, float* values,
                                  uint64_t* active);

/* ---- liquid surface, velocity trails: every particle a chain of shrinking spheres along -velocity ----------------------------------
 * In a splash, spray and thin sheets come out of "liquid surface" as separate round blobs.  OpenVDB's answer is
 * ParticlesToLevelSet::rasterizeTrails (tools/ParticlesToLevelSet.h:649-683, on makeSphere, :713-749): every particle is stamped as
 * a short chain of spheres of decreasing radius behind it, so a fast droplet becomes a tapered streak and a sheet closes up.  This
 * is that loop restated as a function of the particle set, with the trail length accumulated directly in place of |P - P0| and
 * without the library's Rmin / Rmax rejection.  Unchanged from "liquid surface": the constants R, w, dxf, bg, the squared distance
 * x2y2z2 (x2 below) exactly as stated there, and the leaf and list rules.  Float arithmetic unless stated, every operation rounded
 * to float, no FMA; sqrtf and the float division correctly rounded.
 * Settings (fluid_sdf_trails_t): shutter >= 0 and finite, the time the trail covers (shutter = dt: the path of the last step);
 *   delta > 0 and finite, the spacing factor (the library's default: 1); radius_min > 0 and finite, in voxels, the radius at the
 *   trail's end; 1 <= max_instances <= 32; reserved == 0.  Anything else: FLUID_ERR_ARG.  At a snapshot Rm = (float)radius_min must
 *   satisfy Rm <= R, else FLUID_ERR_ARG from the snapshot: R belongs to the call, not to the setting.
 * Instances of a particle with position P0 and velocity v (the handle's doubles; velocities are in the units positions advance in,
 *   x += dt * v: voxels per time, no division by dx):
 *   vf_a = (float)(shutter * v_a) per axis (a double product, one narrowing); s2 = (vf_x*vf_x + vf_y*vf_y) + vf_z*vf_z;
 *   speed = sqrtf(s2).  Instance 0 is (P0, R), always, with P0 untouched.  Unless speed > 0.0f && speed <= FLT_MAX there is no
 *   further instance.  Otherwise inv = 1.0f / speed, n_a = -(vf_a * inv), c = 0.5f * (float)delta, dR = R - Rm, and from t = 0,
 *   r = R, k = 0:  t = t + c * r;  stop unless t <= speed and k + 1 < max_instances;  k = k + 1;  r = R - (dR * t) * inv;  emit the
 *   instance at P_a = P0_a + (double)(t * n_a) (one float product, one double sum) with radius r;  repeat.
 *   Every r <= R (the subtrahend is non-negative).  The loop is bounded by max_instances alone: t may stop growing in float.
 * The voxel.  An instance counts iff its own base cell round(P) lies in [lo,hi]^3: a particle outside the grid can contribute
 *   instances inside it.  For an instance of radius r: mx = r + w, max2 = mx * mx, mn = max(0.0f, r - w), min2 = mn * mn.  Against
 *   voxel c it says nothing if x2 >= max2, INSIDE if x2 <= min2, and otherwise gives the candidate d = dxf * (sqrtf(x2) - r).  The
 *   voxel is inactive -bg if any counted instance says inside; otherwise, with d* the minimum candidate, active with value d* if
 *   d* < bg; inactive +bg in every other case.  An OR and a minimum of floats: order-free, and what makeSphere's order-dependent
 *   sequence leaves in any order (a setValueOff(inside) wins whether it comes before or after a setValue).
 *   When every radius equals R this is "liquid surface" bit for bit: sqrtf, the subtraction of a constant and the product with
 *   dxf > 0 are monotone, so min d = d(min x2).
 * Limits: R + w <= 4 as before; since r <= R an instance within its own mx of a voxel has its base cell within Chebyshev distance 4.
 * Decomposed runs: "liquid surface, velocity trails (decomposed runs)" below.
 * Not built: radii given per particle on the device (fluid_spheres_surface has them on the host), attributes, anisotropic kernels. */
typedef struct fluid_sdf_trails {
    double shutter, delta, radius_min;
    int32_t max_instances, reserved;
} fluid_sdf_trails_t;
/* A setting of the handle beside fluid_sdf_set_surface; NULL clears it.  While it is set, fluid_sdf_snapshot,
 * fluid_sdf_snapshot_filtered, fluid_mesh_snapshot, fluid_mesh_snapshot_filtered, fluid_mesh_snapshot_ex (without
 * FLUID_MESH_VELOCITY) and fluid_render_snapshot take the level set defined above in place of the spheres'; tracks, growth, filter
 * kinds, pack, mesh and ray caster run unchanged.  The range is the box of the counted INSTANCES' base cells, dilated as before;
 * fluid_sdf_grid_t.radius reports R.  Before the kernels are sized the instances' total is read back with their box (8 bytes beside
 * the 24); scratch of 60 bytes per instance is allocated by the first snapshot under the setting.  Cleared: every byte of every
 * entry point what it was.  FLUID_ERR_STATE: on a decomposed handle; while the handle's surface kind is AVERAGED (and
 * fluid_sdf_set_surface(AVERAGED) while trails are set).  Under trails the attribute entry points (fluid_sdf_snapshot_attr,
 * fluid_mesh_snapshot_attr, FLUID_MESH_VELOCITY) and fluid_dist_sdf_snapshot / fluid_dist_sdf_snapshot_attr (on a plain handle)
 * return FLUID_ERR_STATE, as under AVERAGED.  fluid_dist_sdf_snapshot_avg takes its surface as an argument and
 * fluid_dist_sdf_snapshot_trails its trails: they neither read nor are changed by this setting. */
int fluid_sdf_set_trails(fluid_sim_t* s, const fluid_sdf_trails_t* t);
/* Of the last snapshot taken under the setting (either pointer may be NULL): the live particles expanded and the instances made,
 * before the in-grid test. */
int fluid_sdf_trails_stats(fluid_sim_t* s, int64_t* particles, int64_t* instances);
/* Host only, no handle: the expansion above in particle order (pos, vel: x, y, z per particle; vel NULL: all zero) into
 * out_pos[3 * cap] / out_radius[cap].  Returns the instance count (both outputs NULL: the count only, cap is ignored), or
 * -FLUID_ERR_ARG with nothing written: np < 0, a NULL pos with np > 0, p or t NULL or outside their limits, Rm > R, one output NULL
 * alone, cap too small. */
int64_t fluid_particles_trails(int64_t np, const double* pos, const double* vel, const fluid_sdf_params_t* p, const fluid_sdf_trails_t* t,
                               int64_t cap, double* out_pos, float* out_radius);
/* Host only, no handle: the dense level set of n_items arbitrary (position, radius) items by the voxel rule above on the grid of
 * n^3 voxels of size dx: values[n^3] and active[n^3] (z fastest; active may be NULL), brute force over the base cells within 4 of
 * each voxel.  p->radius is the bound R (the limits of p are fluid_sdf_snapshot's); an item with !(0 < radius <= R) is
 * FLUID_ERR_ARG, as are n < 1, !(dx > 0) and a NULL pos or radius (n_items > 0), p or values.  It is how radii per particle are
 * available today, and what k_sdf_search_rad is pinned to bit for bit. */
int fluid_spheres_surface(int32_t n, double dx, int64_t n_items, const double* pos, const float* radius, const fluid_sdf_params_t* p,
                          float* values, uint8_t* active);

/* ---- liquid surface, velocity trails (decomposed runs): a rank record of the rank's own instances, merged exactly ---------------------
 * The trails of "liquid surface, velocity trails" for a FLUID_BLOCKS run.  No new record and no new merge: a rank's record is the
 * plain leaf list (FLUID_SDF_LEAF_BYTES per listed leaf) of the trail surface of the rank's LIVE particles, with their positions and
 * velocities, and the ranks' lists merge through fluid_sdf_grids_merge as it is.
 *
 * The record is exactly what fluid_sdf_snapshot gives under fluid_sdf_set_trails(t) on a one-GPU handle of the same grid that holds
 * the rank's live particles.  Origins are global.  Every leaf the instances reach is listed, whether the rank owns it or not.  An
 * instance counts iff its own base cell lies in the GLOBAL [lo,hi]^3; the rank's block and window play no part in that test, so a
 * trail that leaves the rank's block is whole, and a live particle outside the grid contributes its in-grid instances.  An entry of
 * the rank's arrays that is dead (a served ghost, a particle a sink removed) has a stale position and velocity and no instance.
 * fluid_sdf_grid_t.radius reports R.
 *
 * Why the merge is exact.  A trail voxel of a particle set is inactive -bg if any counted instance says inside; otherwise active
 * with the minimum candidate d* if d* < bg; otherwise inactive +bg.  A rank's list holds, per voxel, that rule over the rank's own
 * instances (a voxel of a leaf a rank does not list is inactive +bg there).  fluid_sdf_grids_merge takes, per voxel over the parts,
 * inactive -bg if any part holds it, else the smallest active value, else inactive +bg.  The instances of the whole set are the
 * disjoint union of the ranks' (every live particle is on exactly one rank, and its instances are a function of it alone), "any
 * instance says inside" is the OR of the ranks' ORs, and where no instance says inside the minimum candidate below bg is the minimum
 * of the ranks' minima below bg (a rank whose own voxel is inside cannot occur then; a rank with no candidate below bg holds +bg,
 * which loses).  A voxel inside on one rank and active on another is -bg in the whole and in the merge.  So the merged list is, byte
 * for byte, what fluid_sdf_snapshot gives under fluid_sdf_set_trails(t) on one handle that holds all ranks' live particles.
 *
 *   per step, every rank:    fluid_step(s, &st);  t.shutter = st.dt_out;  fluid_dist_sdf_snapshot_trails(s, &sp, &t);
 *                            fluid_dist_sdf_wait(s, &part[rank]);
 *   one place:               k = fluid_sdf_grids_merge(part, R, cap, origin, values, active);  filter / mesh / render / write.
 * st.dt_out is the same double on every rank (the step all-reduces the maximum speed before it advects), so shutter = dt is one
 * setting for the whole run.  The rank record is unfiltered and carries no attributes: a block run filters after the merge. */
/* fluid_dist_sdf_snapshot in every respect (live particles only, global coordinates, no transport call, the surface's own two slots
 * and their shared count of outstanding snapshots, survival of a re-balance, a plain record that fluid_dist_sdf_wait takes — and
 * fluid_sdf_wait on a plain fluid_create handle, which is accepted — and fluid_dist_sdf_wait_avg refuses), but the level set is the
 * trails' and they come with the call: t NULL or outside the limits of fluid_sdf_set_trails, or (float)t->radius_min > R:
 * FLUID_ERR_ARG, and no snapshot is outstanding from a refused call.  The handle's surface kind (AVERAGED included) and its own
 * trails setting are neither read nor changed: the surface is the spheres' with these trails.  fluid_dist_sdf_stats reports
 * bytes_to_host = leaves_listed * FLUID_SDF_LEAF_BYTES + 4.  Beside the instances' box and total the live count is read back (8 more
 * bytes); the scratch is that of fluid_sdf_set_trails, shared with it, allocated by the handle's first snapshot of either form. */
int fluid_dist_sdf_snapshot_trails(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_trails_t* t);
/* Of the last fluid_dist_sdf_snapshot_trails (either pointer may be NULL; zeros before the first): the live particles expanded and
 * the instances made, before the in-grid test.  Counters of their own: fluid_sdf_trails_stats keeps reporting the last snapshot
 * under the setting. */
int fluid_dist_sdf_trails_stats(fluid_sim_t* s, int64_t* particles, int64_t* instances);

/* ---- liquid surface as a mesh: surface nets of the level set ----------------------------------------------------------------
 * Polygons for everyone who is no volume renderer.  The reference names tools/VolumeToMesh.h, whose output depends on the library's
 * tree traversal; like the level set itself the mesh gets an exact, order-free definition of its own — naive surface nets on the
 * voxel grid, no case table — and every implementation (the kernels, fluid_sdf_mesh below, the tests' numpy form) gives the same
 * bytes.
 *
 * Input.  The level set of "liquid surface" for the same fluid_sdf_params_t, with the same limits.  val(c), c in [lo,hi]^3, is the
 * value of every voxel, inactive ones included (+bg or -bg); the active mask plays no part.  A voxel is INSIDE iff val(c) < 0.0f.
 *
 * Cells.  Cell c has the corners c + {0,1}^3 and exists iff lo <= c_a <= hi - 1 on every axis: nothing outside the grid is read or
 * assumed.  A cell is MIXED iff its corners are not all inside or all outside.
 *
 * Vertex of a mixed cell (float throughout, no FMA).  Walk the 12 edges in this order: axis a = x, y, z; for each axis the two
 * other axes, in ascending axis order, take the offsets (0,0), (0,1), (1,0), (1,1).  An edge runs from corner c0 (offset 0 on axis
 * a) to c1 = c0 + e_a and COUNTS iff exactly one end is inside.  For a counting edge t = v0 / (v0 - v1) (float subtraction, then the
 * correctly rounded float division); the point's offset from c is t on axis a and the corner's 0.0f / 1.0f on the other two.  One
 * end is < 0 and the other >= 0, so v0 - v1 is never zero and t lies in (0, 1].  Per axis s_axis starts at 0.0f and receives the
 * offsets in edge order; k counts the counting edges.  The vertex is (float)c_axis + s_axis / (float)k, in index space.
 *
 * Quads.  Voxel p owns the edges p -> p + e_a, a = x, y, z.  An edge gives a quad iff its ends differ in sign and the four cells
 * round it exist.  With (b, c) the two other axes in cyclic order (x -> (y,z), y -> (z,x), z -> (x,y)) the cells are Q0 = p - e_b - e_c,
 * Q1 = p - e_c, Q2 = p, Q3 = p - e_b; they exist iff lo <= p_a <= hi - 1 and lo + 1 <= p_b, p_c <= hi - 1, and all four are mixed by
 * construction.  The quad is (Q0, Q1, Q2, Q3) if p is inside — counter-clockwise seen from +a, the normal points out of the liquid —
 * and (Q0, Q3, Q2, Q1) if p is outside; its entries are the cells' vertex numbers (uint32).  Edges that lack a cell (on the outermost
 * voxel layer) give no quad: the mesh is open where the surface meets the grid face.  Degenerate quads are kept.
 *
 * Order.  Vertices ascend by the origin (x, y, z) of the OpenVDB leaf that holds the cell's min corner c, then by c's offset in the
 * leaf ((x&7)*8 + (y&7))*8 + (z&7).  Quads ascend by the leaf origin of p, then p's offset, then a.  Leaf origins are multiples of 8
 * from lo & ~7, as everywhere else.
 *
 * A decomposed run merges its blocks' lists (fluid_sdf_grids_merge) and meshes the result on the host:
 *   k = fluid_sdf_grids_merge(...);  g = {n, k, ...};  nv = fluid_sdf_mesh(&g, 0, 0, NULL, NULL, &nq);  (allocate)  fluid_sdf_mesh(&g, nv, nq, v, q, &nq);
 */
typedef struct fluid_mesh {
    int32_t n;
    int64_t n_vertices, n_quads;
    float radius, half_width, background;   /* R, w, bg as used                                                  */
    const float* vertices;                  /* 3 per vertex, index space                                         */
    const uint32_t* quads;                  /* 4 per quad                                                        */
} fluid_mesh_t;
/* The front half of fluid_sdf_snapshot (box, 24 bytes read back; bins; search) and then the mesh kernels; no leaf is packed.  The
 * search scratch is the surface's: both kinds of snapshot run in order on the handle's stream.  Lifetime rules of the surface
 * snapshot: kernels on the handle's stream, the two totals read back (8 bytes), the records copied to pinned host memory on a second
 * stream and not waited for; two mesh snapshots may be outstanding, a third returns FLUID_ERR_STATE; buffers grow here, never inside
 * a step, and are freed by the destroy call after the copies in flight have ended.  The slots and the count of outstanding snapshots
 * are the mesh's own: density, surface and mesh can all be taken in one step.  Nothing a later step reads is written.
 * FLUID_ERR_ARG: bad parameters (as fluid_sdf_snapshot), or more than 2^31 - 1 vertices or quads.  FLUID_ERR_STATE on a decomposed
 * handle (all three entry points): see fluid_sdf_mesh. */
int fluid_mesh_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p);
/* The oldest snapshot not yet waited for (FLUID_ERR_STATE when there is none).  No counted particle or no mixed cell: counts 0 and
 * NULL pointers (quads is NULL whenever n_quads is 0).  The pointers stay valid until the SECOND following mesh snapshot. */
int fluid_mesh_wait(fluid_sim_t* s, fluid_mesh_t* out);
/* Of the last snapshot (any pointer may be NULL): bytes_to_host = 12 * vertices + 16 * quads + 8 (more for a snapshot with
 * velocities, normals or triangles: "liquid surface, attributes" and "normals and triangles" below). */
int fluid_mesh_stats(fluid_sim_t* s, int64_t* vertices, int64_t* quads, int64_t* bytes_to_host);
/* Host only: the definition above applied to a leaf list, every unlisted leaf being +bg.  Returns the vertex count and *n_quads (may
 * be NULL).  vertices == quads == NULL: the counts only, the caps are ignored; otherwise both arrays are required, 3 * cap_vertices
 * floats and 4 * cap_quads uint32.  -FLUID_ERR_ARG with nothing written: a list fluid_sdf_to_dense refuses, one array without the
 * other, a cap too small, more than 2^31 - 1 vertices or quads.  Works leaf by leaf over the listed leaves and their neighbours at
 * -1; no dense grid is made. */
int64_t fluid_sdf_mesh(const fluid_sdf_grid_t* g, int64_t cap_vertices, int64_t cap_quads, float* vertices, uint32_t* quads, int64_t* n_quads);
/* Host only: binary little-endian PLY, no compression.  Header, line by line: ply / format binary_little_endian 1.0 /
 * element vertex <nv> / property float x / property float y / property float z / element face <nq> /
 * property list uchar uint vertex_indices / end_header.  A vertex is its three index-space components times voxel_size, in float;
 * a face is the byte 4 and the quad's four uint32.  FLUID_ERR_ARG: voxel_size not > 0, a count without its array, a quad entry
 * >= n_vertices, a path that cannot be opened or written in full (the partial file is removed). */
int fluid_write_ply_mesh(const char* path, const fluid_mesh_t* m, float voxel_size);

/* ---- liquid surface, attributes: the closest particle's id and velocity per voxel, a velocity per mesh vertex (single GPU) -------
 * Geometry alone leaves the device above.  Motion blur needs a velocity per vertex; colour, age or foam need to know which
 * particle a piece of surface belongs to.  OpenVDB's ParticlesToLevelSet has the second half (the AttributeT template argument,
 * attributeGrid(), getAtt and Merge(d, att), tools/ParticlesToLevelSet.h:132-189, 603-637): every voxel the rasteriser sets also
 * receives the attribute of the particle that set it.  Like the level set, the mesh and the filter this gets an exact, order-free
 * definition of its own, and the kernels, the host functions below and the tests' numpy form give the same bytes.  Float unless
 * stated, no FMA.
 *
 * Voxel attributes.  Input: the level set of "liquid surface" for the same fluid_sdf_params_t, the same counted particles, the
 * same x2y2z2.  For an ACTIVE voxel c, m(c) is the minimum of x2y2z2 over the counted particles, as there.
 *   The voxel's closest particle is the counted particle with x2y2z2 == m(c) that has the SMALLEST id.
 *   id(c) is that particle's id: on a one-GPU handle the row of the particle in what fluid_download_particles returns at the time
 *   of the snapshot (the ids given to fluid_upload_particles_ids, where that was the upload).
 *   vel(c) = ((float)vx, (float)vy, (float)vz) of that particle: one narrowing of the handle's double velocity, no scaling.
 *   A voxel that is not active (inactive +-bg, or outside the grid in a listed leaf) has id = FLUID_SDF_NO_ID and
 *   vel = (+0.0f, +0.0f, +0.0f).
 * No particle order is involved.  Every particle with the minimal x2y2z2 also has the minimal d, so this is the attribute grid the
 * library leaves when it happens to visit that particle first (`if (d < v)` is strict, :637): it is ONE OF the library's possible
 * outcomes, not "the" outcome — the library's depends on the order of its particle list.  The tie is broken on m, not on d: many
 * distinct m share one d (up to 40 float steps of m for valid parameters), and a single pass cannot know the final class of d
 * while it walks.
 * A filter (fluid_sdf_filter_t) changes values, never topology: ids and velocities of a filtered snapshot are those of the
 * unfiltered one, as in the library, where LevelSetFilter never touches the attribute grid.
 *
 * Vertex velocity.  Take a mixed cell's vertex and walk its 12 edges in the order of "liquid surface as a mesh".  For every
 * COUNTING edge, with v0, v1, t as defined there, A0, A1 the active bits of its two ends and a0, a1 their velocity component:
 *   both ends active:      e = a0 + t * (a1 - a0)   (float subtract, multiply, add);
 *   only one end active:   e = that end's component;
 *   neither end active:    the edge contributes nothing.
 * Per component s starts at 0.0f and receives the e in edge order; kv counts the contributing edges.  The component is
 * s / (float)kv, or +0.0f when kv == 0.  Vertex order is the mesh's.
 * An edge with no active end cannot come from a device snapshot: an inactive -bg voxel (distance <= R - w) and an inactive +bg
 * voxel (distance >= R + w) are 2w >= 2 apart, grid neighbours differ by at most 1, and the filter leaves inactive voxels alone.
 * Only a hand-made leaf list reaches that rule: fluid_sdf_mesh_attr implements it, the kernel carries the same rule and cannot be
 * driven into it.  One-ended edges do occur after a filter (the filter moves the sign change into the band's rim).
 *
 * Decomposed handles get FLUID_ERR_STATE from the four handle entry points below: a block run takes a record per rank that also
 * carries m and merges the records on the host ("liquid surface, attributes (decomposed runs)", below). */
#define FLUID_SDF_NO_ID 0xffffffffu
typedef struct fluid_sdf_attr {
    int32_t n_leaves;
    const uint32_t* id;          /* 512 per leaf, the order of fluid_sdf_grid_t.values                               */
    const float* velocity;       /* [leaf][axis][512]                                                                */
} fluid_sdf_attr_t;
#define FLUID_SDF_ATTR_LEAF_BYTES (2048 + 6144)   /* what the attributes add to a listed leaf on the way to the host   */
typedef struct fluid_mesh_attr {
    int64_t n_vertices;
    const float* velocity;       /* 3 per vertex, the handle's velocity units                                        */
} fluid_mesh_attr_t;
/* fluid_sdf_snapshot (f == NULL) or fluid_sdf_snapshot_filtered (f != NULL) in every respect — same two slots, same copy stream,
 * same count of outstanding snapshots (a third is FLUID_ERR_STATE), same fluid_sdf_stats —, and the values, masks and origins are
 * byte for byte those of the plain snapshot; the record that travels behind the same event is longer by the ids and velocities:
 * bytes_to_host = leaves_listed * (FLUID_SDF_LEAF_BYTES + FLUID_SDF_ATTR_LEAF_BYTES) + 4.  The extra scratch (4 B per particle,
 * 8 KB per leaf of the range) is allocated by the handle's first attribute snapshot, surface or mesh, never inside a step; a
 * caller that never asks for attributes allocates nothing more.  Nothing a later step reads is written. */
int fluid_sdf_snapshot_attr(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f);
/* fluid_sdf_wait, and the attributes of the same snapshot (attr may be NULL).  A snapshot taken without attributes, or with no
 * listed leaf, gives NULL attribute pointers (n_leaves is the grid's).  fluid_sdf_wait on an attribute snapshot returns the
 * geometry alone.  Lifetime of the pointers: that of the grid's. */
int fluid_sdf_wait_attr(fluid_sim_t* s, fluid_sdf_grid_t* grid, fluid_sdf_attr_t* attr);
/* fluid_mesh_snapshot (f == NULL: the box dilated by 4) or fluid_mesh_snapshot_filtered (f != NULL: by 5) with a velocity per
 * vertex: same slots, stream, count and fluid_mesh_stats, vertices and quads byte for byte the plain ones;
 * bytes_to_host = 24 * vertices + 16 * quads + 8. */
int fluid_mesh_snapshot_attr(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f);
/* fluid_mesh_wait, and the vertex velocities (attr may be NULL); NULL velocity for a snapshot taken without attributes or with no
 * vertex.  fluid_mesh_wait on an attribute snapshot returns the geometry alone. */
int fluid_mesh_wait_attr(fluid_sim_t* s, fluid_mesh_t* mesh, fluid_mesh_attr_t* attr);
/* Host only: the vertex velocities of fluid_sdf_mesh(grid), in its vertex order, into velocity[3 * cap_vertices]; grid->values
 * may be filtered values.  Returns the vertex count (velocity == NULL: the count only, the cap is ignored), or -FLUID_ERR_ARG
 * with nothing written: a list fluid_sdf_to_dense refuses, attr NULL or attr->n_leaves != grid->n_leaves, leaves without the
 * attribute arrays, a cap too small.  Works leaf by leaf with bisection for the neighbours, as fluid_sdf_mesh; no dense grid. */
int64_t fluid_sdf_mesh_attr(const fluid_sdf_grid_t* grid, const fluid_sdf_attr_t* attr, int64_t cap_vertices, float* velocity);
/* Host only: id[n^3] = FLUID_SDF_NO_ID and velocity[3 * n^3] ([axis][n^3], z fastest) = +0.0f everywhere, then the in-grid voxels
 * of every listed leaf (either array may be NULL).  FLUID_ERR_ARG as fluid_sdf_to_dense, and for a leaf-count mismatch. */
int fluid_sdf_attr_to_dense(const fluid_sdf_grid_t* grid, const fluid_sdf_attr_t* attr, uint32_t* id, float* velocity);
/* Host only: fluid_write_ply_mesh with `property float vx / vy / vz` after `property float z`: a vertex record is six floats, the
 * position times voxel_size and the velocity components times velocity_scale, both in float.  FLUID_ERR_ARG as there, and for
 * attr NULL, attr->n_vertices != m->n_vertices, vertices without velocities, or a velocity_scale that is not finite. */
int fluid_write_ply_mesh_attr(const char* path, const fluid_mesh_t* m, const fluid_mesh_attr_t* attr, float voxel_size, float velocity_scale);

/* ---- liquid surface, attributes (decomposed runs) -----------------------------------------------------------------------------
 * No new arithmetic: m(c), x2y2z2, "counted", "live" and the closest-particle rule are those of the sections above.  A merge that
 * looks at values cannot be exact — equal values do not imply equal m (many m share one d), and with equal m the smaller id may sit
 * on any rank — so the rank record carries m itself and the merge decides on it.
 *
 * Rank record.  The attribute snapshot of a rank is fluid_dist_sdf_snapshot's list for this rank's LIVE particles: origins, values
 * and masks are byte for byte the plain snapshot's.  Per voxel it adds id, velocity and dist2:
 *   ACTIVE voxel:       id and velocity as in "liquid surface, attributes", taken over this rank's live particles — the ids are
 *                       the handle's global ids, as fluid_download_particles_ids returns them —, and dist2 = m(c) over those
 *                       particles, as a float;
 *   every other voxel:  FLUID_SDF_NO_ID, +0.0f velocity, dist2 = +infinity (bit pattern 0x7f800000).
 *
 * Merge.  Geometry follows the three-state rule of "liquid surface (decomposed runs)", unchanged: origins, values and masks are
 * the bytes fluid_sdf_grids_merge gives.  Attributes of a voxel whose merged state is active: among the parts that hold it active
 * take the smallest dist2; among equal dist2 the smallest id; among equal id the first part (a device run cannot produce this
 * case: a particle is live on one rank only).  id and velocity are that part's.  Every other voxel gets FLUID_SDF_NO_ID and +0.0f.
 * Exact: a minimum over a union is the minimum of the minima; d is monotone in m, so the part with the smallest dist2 also holds
 * the smallest active value; a voxel that is -bg on any part is -bg in the union.  For the records the ranks of a run give, the
 * result is what fluid_sdf_snapshot_attr gives on one handle that holds the union of their live particles with the same ids.
 *
 *   per step, every rank:    fluid_step(s, &st);  fluid_dist_sdf_snapshot_attr(s, &sp);  fluid_dist_sdf_wait_attr(s, &part[rank], &rec[rank]);
 *   one place:               k = fluid_sdf_attr_grids_merge(part, rec, R, cap, origin, values, active, id, velocity);
 *                            g = {n, k, ...};  a = {k, id, velocity};  fluid_sdf_filter / fluid_sdf_mesh / fluid_sdf_mesh_attr as on one GPU.
 * The rank snapshot is unfiltered, as its sibling: a block run filters after the merge, and a filter leaves attributes alone. */
typedef struct fluid_sdf_attr_part {
    int32_t n_leaves;
    const uint32_t* id;          /* 512 per leaf                                                                     */
    const float* velocity;       /* [leaf][axis][512]                                                                */
    const float* dist2;          /* 512 per leaf                                                                     */
} fluid_sdf_attr_part_t;
#define FLUID_SDF_ATTR_PART_LEAF_BYTES (2048 + 6144 + 2048)   /* what a rank record adds to a listed leaf on the way to the host */
/* fluid_dist_sdf_snapshot in every respect — stream, the box and the 4-byte count read back, the copy stream, the surface's own two
 * slots and its count of outstanding snapshots (a third, of whatever kind, is FLUID_ERR_STATE) — with the longer record:
 * fluid_dist_sdf_stats reports bytes_to_host = leaves_listed * (FLUID_SDF_LEAF_BYTES + FLUID_SDF_ATTR_PART_LEAF_BYTES) + 4.  A plain
 * fluid_create handle is accepted; its ids are rows of fluid_download_particles (or the ids of fluid_upload_particles_ids).  The
 * extra scratch (that of fluid_sdf_snapshot_attr and 2 KB more per leaf of the range) is allocated by the handle's first snapshot
 * of this kind, never inside a step; no other caller pays for it. */
int fluid_dist_sdf_snapshot_attr(fluid_sim_t* s, const fluid_sdf_params_t* p);
/* fluid_dist_sdf_wait, and the record of the same snapshot (part may be NULL).  A snapshot taken by any other call, or one with no
 * listed leaf, gives NULL record pointers (n_leaves is the grid's).  fluid_dist_sdf_wait on such a snapshot returns the geometry
 * alone.  Lifetime of the pointers: that of the grid's, also across a step that moves the cut planes. */
int fluid_dist_sdf_wait_attr(fluid_sim_t* s, fluid_sdf_grid_t* grid, fluid_sdf_attr_part_t* part);
/* Host only.  The merge defined above: origin / values / active as fluid_sdf_grids_merge, id[512 * cap_leaves] and
 * velocity[1536 * cap_leaves] ([leaf][axis][512]) beside them.  Returns the merged leaf count (all five outputs NULL: the count only,
 * cap_leaves is ignored; otherwise all five are required), or -FLUID_ERR_ARG with nothing written: every refusal of
 * fluid_sdf_grids_merge; attrs NULL or attrs[i].n_leaves != parts[i].n_leaves; leaves without the three record arrays; an active
 * voxel of a part with a dist2 that is not finite or with FLUID_SDF_NO_ID; a voxel where the part with the smallest dist2 does not
 * hold the smallest active value as a bit pattern (only a hand-made list reaches this).  Parts with n_leaves == 0 and NULL pointers
 * are valid.  Two passes over a k-way merge of the ascending lists; no dense grid. */
int64_t fluid_sdf_attr_grids_merge(const fluid_sdf_grid_t* parts, const fluid_sdf_attr_part_t* attrs, int32_t n_parts, int64_t cap_leaves,
                                   int32_t* origin, float* values, uint64_t* active, uint32_t* id, float* velocity);

/* ---- liquid surface as a mesh: normals and triangles ------------------------------------------------------------------------------
 * Game engines and most realtime viewers take triangles and want a shading normal per vertex; face normals recomputed from a
 * surface-nets mesh show facets.  The level set's gradient IS the normal, and the emit kernel holds the cell's eight corner values
 * at the moment it writes the vertex.  Both are options of the mesh: with them off every byte and every stat is what it was.  Like
 * the mesh itself they are exact and order-free: the kernels, the host functions below and the tests' numpy form (tests/
 * mesh_normals_ref.py) are compared with ==.  Float throughout, no FMA; division and sqrtf are the correctly rounded IEEE operations;
 * denormals are kept.
 *
 * Normal of a mixed cell's vertex.  f_axis = s_axis / (float)k is the vertex's offset in its cell, exactly as "liquid surface as a
 * mesh" forms it before (float)c_axis is added (NOT vertex - c, which differs by the rounding of that add).  The normal is the
 * gradient of the trilinear interpolant of the cell's eight corner values val(c + {0,1}^3) — inactive +-bg included, filtered values
 * after a filter, the active mask plays no part — at f, normalised.  For axis a = x, y, z, with b1 < b2 the two other axes:
 *   g_a = 0.0f
 *   for (d1, d2) in (0,0), (0,1), (1,0), (1,1):                 (the mesh's edge order)
 *       w1 = d1 ? f_b1 : (1.0f - f_b1);   w2 = d2 ? f_b2 : (1.0f - f_b2)
 *       g_a = g_a + (w1 * w2) * (v1 - v0)                        (v0: the corner at (d1, d2) on (b1, b2) and 0 on a; v1: 1 on a)
 *   l2 = g_x * g_x;  l2 = l2 + g_y * g_y;  l2 = l2 + g_z * g_z;  len = sqrtf(l2)
 *   n_a = (len > 0.0f) ? g_a / len : +0.0f                       (all three components; a NaN length gives +0 too)
 * Values are negative inside, so the normal points out of the liquid, as the quads' winding does.  All 12 edges enter, not only the
 * counting ones.  Order: the mesh's vertex order.
 * Stated limit: corners further than w from the surface are clamped to +-bg, so with w = 1 the direction is slightly biased in cells
 * whose far corners sit on the plateau; w >= 2 avoids it.  On sheets thinner than a cell (under-resolved surface nets) a normal may
 * oppose its quads' winding.  A central-difference gradient over a wider tile is not offered.
 *
 * Triangles.  Quad i with entries (a, b, c, d) gives triangles 2i and 2i + 1, cut along the shorter diagonal of the vertex positions
 * in index space:  d02 = |V_c - V_a|^2, d13 = |V_d - V_b|^2, each as dx*dx, then + dy*dy, then + dz*dz over float differences;
 *   d13 < d02:  (a, b, d), (b, c, d);      otherwise (ties and NaN):  (a, b, c), (a, c, d).
 * The winding is the quad's, degenerate triangles are kept, the entries are uint32 vertex numbers: exactly 2 * n_quads triangles, in
 * quad order.
 *
 * A decomposed run: mesh the merged list (fluid_sdf_mesh), then fluid_sdf_mesh_normals(&g, nv, normals) and
 * fluid_mesh_triangles(&mesh, 2 * nq, triangles). */
#define FLUID_MESH_VELOCITY  1u
#define FLUID_MESH_NORMALS   2u
#define FLUID_MESH_TRIANGLES 4u
typedef struct fluid_mesh_ex {
    const float* velocity;       /* 3 per vertex ("liquid surface, attributes"), or NULL                             */
    const float* normals;        /* 3 per vertex, unit length or +0, or NULL                                         */
    const uint32_t* triangles;   /* 3 per triangle, or NULL                                                          */
    int64_t n_triangles;         /* 2 * n_quads with triangles, else 0                                               */
} fluid_mesh_ex_t;
/* fluid_mesh_snapshot / _filtered / _attr with any of the three parts: what = 0 is fluid_mesh_snapshot (f == NULL) or
 * fluid_mesh_snapshot_filtered (f != NULL), what = FLUID_MESH_VELOCITY is fluid_mesh_snapshot_attr.  Same slots, stream, count of
 * outstanding snapshots and range (the box dilated by 4 without a filter, 5 with one); vertices and quads are byte for byte the plain
 * ones.  The record that travels is [quads | 24 B of triangles per quad | vertices | velocities | normals], each part only if asked
 * for: the triangles start at a multiple of 16 for every count, so the kernel writes each quad's pair with one 16-byte and one
 * 8-byte store.  fluid_mesh_stats: bytes_to_host = 16 nq + 12 nv (1 + velocity + normals) + 24 nq triangles + 8.  No scratch beyond
 * what `what` asks for (velocities alone need the attribute scratch).  FLUID_ERR_ARG: as the siblings, or unknown bits in `what`.
 * FLUID_ERR_STATE on a decomposed handle (both entry points): see the two host functions below. */
int fluid_mesh_snapshot_ex(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f /* NULL: unfiltered */, uint32_t what);
/* fluid_mesh_wait, and the parts of the same snapshot (ex may be NULL): NULL for every part the snapshot was taken without, for
 * velocity and normals with no vertex, for triangles with no quad.  fluid_mesh_wait and fluid_mesh_wait_attr on such a snapshot
 * return what they know (the geometry; the velocity).  Lifetime of the pointers: that of the mesh's. */
int fluid_mesh_wait_ex(fluid_sim_t* s, fluid_mesh_t* mesh, fluid_mesh_ex_t* ex);
/* Host only: the vertex normals of fluid_sdf_mesh(grid), in its vertex order, into normals[3 * cap_vertices]; grid->values may be
 * filtered values.  Returns the vertex count (normals == NULL: the count only, the cap is ignored), or -FLUID_ERR_ARG with nothing
 * written: a list fluid_sdf_to_dense refuses, a cap too small, more than 2^31 - 1 vertices.  Works leaf by leaf with bisection for
 * the neighbours, as fluid_sdf_mesh; no dense grid. */
int64_t fluid_sdf_mesh_normals(const fluid_sdf_grid_t* grid, int64_t cap_vertices, float* normals);
/* Host only: the triangles of any mesh into triangles[3 * cap_triangles].  Returns 2 * n_quads (triangles == NULL: the count only,
 * the cap is ignored), or -FLUID_ERR_ARG with nothing written: mesh NULL, negative counts, a count without its array, a quad entry
 * >= n_vertices, a cap too small, more than 2^31 - 1 quads. */
int64_t fluid_mesh_triangles(const fluid_mesh_t* mesh, int64_t cap_triangles, uint32_t* triangles);
/* Host only: fluid_write_ply_mesh / _attr with any of the parts of ex (NULL, or all parts NULL: fluid_write_ply_mesh's bytes).  The
 * vertex record is x y z [nx ny nz] [vx vy vz]: `property float nx / ny / nz` after z, the normals unscaled; then vx / vy / vz times
 * velocity_scale.  With ex->triangles the faces are `element face <2 nq>`, each the byte 3 and three uint32, instead of the quads;
 * otherwise the quads are written as there.  FLUID_ERR_ARG as the siblings, and for n_triangles != 2 * n_quads with triangles, a
 * triangle entry >= n_vertices, a velocity_scale that is not finite with velocities. */
int fluid_write_ply_mesh_ex(const char* path, const fluid_mesh_t* m, const fluid_mesh_ex_t* ex, float voxel_size, float velocity_scale);

/* ---- liquid surface as an image: a ray caster for the level set -----------------------------------------------------------------
 * What the reference delivers is pictures: OpenVDB's vdb_render over the files its run wrote.  The level set sits on the device after
 * the front half of a surface snapshot, one launch away from an image.  Like the surface, the filter, the mesh and the normals the
 * image gets an exact, order-free definition of its own, restated from the library's LinearSearchImpl (tools/RayIntersector.h:539-692:
 * uniform steps, the first sign change, one linear interpolation of the hit time) and DiffuseShader; the kernels
 * (kernels_render.hip), fluid_sdf_render below and the tests' numpy form (tests/render_ref.py) give the same bytes.  Float throughout,
 * no FMA; / and sqrtf are the correctly rounded IEEE operations; denormals are kept.
 *
 * Input.  The level set of "liquid surface" for a fluid_sdf_params_t, optionally after a fluid_sdf_filter_t: val(c), c in [lo,hi]^3,
 * inactive voxels included (+-bg).  Every voxel of an unlisted leaf and every voxel outside the grid is +bg.  The active mask plays
 * no part.
 *
 * Camera (fluid_camera_t, index space).  Pixel (i, j) = column i, row j, row 0 first (as in a PNG); its record index is j * width + i.
 *   pi = (float)i + 0.5f;  pj = (float)j + 0.5f
 *   D_a = (dir00_a + pi * du_a) + pj * dv_a                                    (grouped as written)
 *   l2 = D_x * D_x;  l2 = l2 + D_y * D_y;  l2 = l2 + D_z * D_z;  len = sqrtf(l2)
 *   !(len > 0.0f) or len not finite: the pixel is a MISS.  Otherwise d_a = D_a / len.
 * A pinhole, an orthographic camera (du, dv chosen by the caller) and anything between are the caller's numbers; no trigonometry
 * crosses the ABI (fluid_camera_look_at below is a convenience on top).
 *
 * Value at a point p.  If any p_a is NaN, or p_a < (float)(lo - 1), or p_a >= (float)(hi + 1): value(p) = +bg, the constant, no
 * arithmetic.  Otherwise c_a = (int)floorf(p_a), which lies in [lo - 1, hi], f_a = p_a - (float)c_a in [0, 1], the corners
 * v[dx][dy][dz] = val(c + (dx, dy, dz)) (+bg outside the grid), lerp(a, b, t) = a + t * (b - a) (a subtraction, a multiplication, an
 * addition), and the value is four lerps along z with f_z (in the order (dx, dy) = (0,0), (0,1), (1,0), (1,1)), then two along y
 * with f_y, then one along x with f_x.
 *
 * March.  t_k = t_near + (float)k * step,  p_k,a = eye_a + t_k * d_a,  k = 0 .. n_steps - 1.  The pixel HITS at the smallest k with
 * value(p_k) < 0.0f; with none it is a miss.  k = 0 (the eye is in the liquid): t = t_0.  Otherwise v0 = value(p_{k-1}),
 * v1 = value(p_k) and  t = t_{k-1} + ((t_k - t_{k-1}) * v0) / (v0 - v1)  (the library's interpTime; no iteration of the hit).  v0 >= 0 >
 * v1, so the divisor is positive.
 *
 * Normal at the hit.  p_h,a = eye_a + t * d_a.  If p_h is out of bounds by the rule of value(): (+0, +0, +0).  Otherwise the cell c and
 * f as in value(), and the g_a / l2 / len / n_a formula of "normals and triangles", unchanged, on that cell's eight corners at f.
 *
 * Outputs per pixel.  depth: t, or +infinity (0x7f800000) on a miss.  normal: n, or +0 on a miss.  rgb from fluid_shade_t: a miss takes
 * `background`; a hit  s = n_x * d_x;  s = s + n_y * d_y;  s = s + n_z * d_z;  s = fabsf(s)  (DiffuseShader), per channel
 * x = base_c * s clamped to [0, 1] (x > 0 ? (x < 1 ? x : 1) : 0, so NaN gives 0), byte = (uint8_t)(x * 255.0f + 0.5f).  n_hit counts
 * the hit pixels.
 *
 * Skipping empty space changes nothing.  For a, b >= 0 and t in [0, 1], lerp(a, b, t) >= 0 in float: t * |b - a| <= max(a, b) survives
 * the rounding of the product and of the sum (tests/test_render_ref.py tries 2 M triples, denormals and t = 1 - ulp included).  So a
 * cell whose eight corners are all >= 0 never gives the first negative sample, and an implementation may leave out every sample that
 * is out of bounds or whose cell lies in a leaf L with no negative voxel in L + {0,1}^3.  Only v0 at a hit must then be evaluated by
 * the formula: one more value() per hit pixel.  Per axis p_k,a is monotone in k (every operation that forms it is), so the samples
 * between two samples of one axis-aligned box lie in that box.
 *
 * What this is not.  No voxel DDA (math/DDA.h): the march is uniform in t, a feature thinner than `step` can be stepped over, and
 * step <= 0.5 is the advice.  No iteration of the hit, no shadows, no refraction, no solids, no colour by velocity, no anti-aliasing
 * (render larger and average).
 * Limits (anything else is FLUID_ERR_ARG): width, height in 1..8192 and width * height <= 2^24; n_steps in 1..65536; step > 0 and
 * t_near >= 0; every camera float and every `base` finite; pad_ == 0; `what` non-zero and within the three bits. */
typedef struct fluid_camera {
    float eye[3], dir00[3], du[3], dv[3];
    int32_t width, height;
    float t_near, step;
    int32_t n_steps;
} fluid_camera_t;
typedef struct fluid_shade { float base[3]; uint8_t background[3]; uint8_t pad_; } fluid_shade_t;
#define FLUID_RENDER_RGB     1u
#define FLUID_RENDER_DEPTH   2u
#define FLUID_RENDER_NORMALS 4u
typedef struct fluid_image {
    int32_t width, height;
    int64_t n_hit;
    const uint8_t* rgb;          /* 3 per pixel, or NULL                                                             */
    const float* depth;          /* 1 per pixel, or NULL                                                             */
    const float* normals;        /* 3 per pixel, or NULL                                                             */
} fluid_image_t;
/* The front half of fluid_sdf_snapshot (box, 24 bytes read back; bins; search; with f the box passes, over the box dilated by 5 as for
 * a filtered mesh: a negative voxel is active or -bg, so a cell with a negative corner has its min corner in [-5, +4] of a base cell),
 * then the render kernels on the handle's stream; no leaf is packed.  shade == NULL: base (1, 1, 1) on a black background.  The record
 * [16 bytes: uint32 hits and three zero words | rgb, padded to a multiple of 16 | depth | normals], each part only if asked for,
 * travels to pinned host memory on a second stream and is not waited for; the hit count is an integer sum in the record's header, so
 * there is no host wait beyond the front half's box.  The slots and the count of outstanding snapshots are the image's own: density,
 * surface, mesh and image can all be taken in one step; two may be outstanding, a third returns FLUID_ERR_STATE.  Buffers grow here,
 * never inside a step, and are freed by the destroy call after the copies in flight have ended.  With no counted particle every pixel
 * is a miss and the record is produced all the same.  Nothing a later step reads is written.  FLUID_ERR_ARG: bad parameters or filter
 * (as the siblings), a limit above.  FLUID_ERR_STATE on a decomposed handle (all three entry points): see fluid_sdf_render. */
int fluid_render_snapshot(fluid_sim_t* s, const fluid_sdf_params_t* p, const fluid_sdf_filter_t* f /* NULL: unfiltered */,
                          const fluid_camera_t* cam, const fluid_shade_t* shade, uint32_t what);
/* The oldest snapshot not yet waited for (FLUID_ERR_STATE when there is none); parts not asked for are NULL.  The pointers stay valid
 * until the SECOND following render snapshot on the handle. */
int fluid_render_wait(fluid_sim_t* s, fluid_image_t* out);
/* pixels = width * height and bytes_to_host = 16 + pad16(3 W H) [rgb] + 4 W H [depth] + 12 W H [normals] of the last snapshot TAKEN;
 * hits of the last snapshot WAITED FOR (the count travels with the record; 0 before the first wait).  Any pointer may be NULL. */
int fluid_render_stats(fluid_sim_t* s, int64_t* pixels, int64_t* hits, int64_t* bytes_to_host);
/* Host only: the definition above applied to a leaf list (grid->values may be filtered values), every sample evaluated, the leaves
 * found by bisection; no dense grid.  How a block run renders: after fluid_sdf_grids_merge (and fluid_sdf_filter).  rgb[3 W H],
 * depth[W H], normals[3 W H]: required for the parts `what` names, ignored otherwise; n_hit may be NULL; shade == NULL as above.
 * FLUID_ERR_ARG with nothing written: a list fluid_sdf_to_dense refuses, a limit above, a part asked for without its array. */
int fluid_sdf_render(const fluid_sdf_grid_t* grid, const fluid_camera_t* cam, const fluid_shade_t* shade, uint32_t what, uint8_t* rgb,
                     float* depth, float* normals, int64_t* n_hit);
/* Host only, a convenience: the pinhole camera of a grid of n^3 cells that looks from `eye` at `target` (index space) with `up`
 * roughly upwards and a vertical field of view of fov_y_degrees; square pixels, row 0 at the top.  Computed in double and narrowed
 * once; t_near = 0, n_steps just enough to pass the grid's farthest corner (at most 65536).  Not pinned bit for bit (libm's tan).
 * FLUID_ERR_ARG: n < 1, a non-finite input, eye == target, up parallel to the view, fov outside (0, 180), width or height outside
 * 1..8192 or more than 2^24 pixels, step not > 0. */
int fluid_camera_look_at(int32_t n, const double eye[3], const double target[3], const double up[3], double fov_y_degrees, int32_t width,
                         int32_t height, double step, fluid_camera_t* out);
/* Host only: an 8-bit RGB PNG, filter type 0 on every row, one IDAT chunk through zlib.  The file's bytes depend on zlib's version;
 * its pixels do not.  FLUID_ERR_ARG: width or height outside 1..8192, rgb NULL, a path that cannot be opened or written in full (the
 * partial file is removed). */
int fluid_write_png(const char* path, int32_t width, int32_t height, const uint8_t* rgb);

#ifdef __cplusplus
}
#endif
#endif /* FLUID_HIP_H */
