// Particle sources and sinks for gfx950 (wave64, 256-thread blocks): the reference's commented-out emitter
// (fluid.cc:1374-1375, 1495-1497) and its general form, applied at the end of a one-GPU step (fluid_sources.hip) and of a
// block-decomposed step (fluid_dist.hip) by the same kernels: a source box and `linear` are GLOBAL, the solid bytes of the box
// come through a SolidView, the cells a handle emits are those of its OwnBox, and a one-GPU handle is the whole-grid window
// (origin 0, dims N, owned [0, N), no dead particle).
//
// Everything here is integer-exact or a fixed function of its inputs: the FILL histogram counts with integer atomics,
// the emitted points come from a counter-based hash of (seed, t, cell, k) and land at offsets given by an exclusive scan
// in cell order, and the sink compaction is a stable scan in device order with the pids renumbered by a scan in pid order.
#include "common.h"
#include "dist_kernels.h"

namespace fl {

// Point k of cell (cx, cy, cz) (coordinates) with cell hash h = sm(sm(sm(seed) ^ t) ^ linear); true iff it is kept.
__device__ __forceinline__ bool src_point(uint64_t h, int k, int cx, int cy, int cz, double& px, double& py, double& pz)
{
    const uint64_t key = h ^ (uint64_t)k;
    const double s = 1.0 / 9007199254740992.0;   // 2^-53
    px = (double)cx + ((double)(sm64(key + 0) >> 11) * s - 0.5);
    py = (double)cy + ((double)(sm64(key + 1) >> 11) * s - 0.5);
    pz = (double)cz + ((double)(sm64(key + 2) >> 11) * s - 0.5);
    return round(px) == (double)cx && round(py) == (double)cy && round(pz) == (double)cz;
}

// base cell round(p) inside the inclusive index box b (compared as doubles: NaN or far-off positions are in no box)
__device__ __forceinline__ bool in_box(const Grid& g, const Box& b, double x, double y, double z, int& lx, int& ly, int& lz)
{
    const double rx = round(x) - (double)g.lo, ry = round(y) - (double)g.lo, rz = round(z) - (double)g.lo;
    if (!(rx >= b.x0 && rx <= b.x1 && ry >= b.y0 && ry <= b.y1 && rz >= b.z0 && rz <= b.z1)) return false;
    lx = (int)rx - b.x0, ly = (int)ry - b.y0, lz = (int)rz - b.z0;
    return true;
}

// ---- FILL: live particles per base cell of the source box (a decomposed run sums the ranks' histograms) --------------------
// skip_dead (launch-uniform): the arrays hold dead entries (PID_DEAD: served ghosts, migrants, what a sink took) among the live
// ones; without it pid[] is not read
__global__ __launch_bounds__(256) void k_src_count(Grid g, long n, Particles p, Box box, int* __restrict__ hist, int skip_dead)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (skip_dead && p.pid[i] == PID_DEAD)) return;
    int lx, ly, lz;
    if (in_box(g, box, p.px[i], p.py[i], p.pz[i], lx, ly, lz)) atomicAdd(hist + ((long)lx * box.ny() + ly) * box.nz() + lz, 1);
}

// ---- kept points per cell of the box (box-local z-fastest order = ascending global linear order) ---------------------
struct SrcArgs {
    uint64_t h0;     // sm(sm(seed) ^ t)
    int per_cell, fill;
};
// tries of box cell l = global index cell (ix, iy, iz)
__device__ __forceinline__ int src_tries(int N, const Box& box, const SrcArgs& a, const SolidView& sv, const int* hist, long l, int& ix, int& iy,
                                         int& iz)
{
    const int nz = box.nz(), ny = box.ny();
    iz = box.z0 + (int)(l % nz);
    iy = box.y0 + (int)((l / nz) % ny);
    ix = box.x0 + (int)(l / ((long)nz * ny));
    const int w0 = 2, w1 = N - 3;   // W in index space
    if (ix < w0 || ix > w1 || iy < w0 || iy > w1 || iz < w0 || iz > w1) return 0;
    if (sv.p[(ix - sv.o[0]) * sv.sx + (iy - sv.o[1]) * sv.sy + (iz - sv.o[2])]) return 0;
    return a.fill ? max(0, a.per_cell - hist[l]) : a.per_cell;
}
__device__ __forceinline__ uint64_t src_cell_hash(int N, const SrcArgs& a, int ix, int iy, int iz)
{
    return sm64(a.h0 ^ (uint64_t)(((size_t)ix * N + (size_t)iy) * N + (size_t)iz));   // `linear` of the global grid
}
__device__ __forceinline__ bool owns_cell(const OwnBox& ob, int ix, int iy, int iz)
{
    return ix >= ob.lo[0] && ix < ob.hi[0] && iy >= ob.lo[1] && iy < ob.hi[1] && iz >= ob.lo[2] && iz < ob.hi[2];
}

// Every handle plans the whole box: cnt = kept points per cell (the same array on every rank: its scan numbers the ids),
// cnt_own = the same where this handle owns the cell, else 0 (its scan places the points in this handle's arrays); nullptr
// (launch-uniform) when it owns every cell of the box: cnt is both
__global__ __launch_bounds__(256) void k_src_plan(Grid g, Box box, SrcArgs a, OwnBox ob, SolidView sv, const int* __restrict__ hist,
                                                  int* __restrict__ cnt, int* __restrict__ cnt_own)
{
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= box.cells()) return;
    int ix, iy, iz;
    const int m = src_tries(g.N, box, a, sv, hist, l, ix, iy, iz);
    int kept = 0;
    if (m > 0) {
        const uint64_t h = src_cell_hash(g.N, a, ix, iy, iz);
        double px, py, pz;
        for (int k = 0; k < m; ++k) kept += src_point(h, k, g.lo + ix, g.lo + iy, g.lo + iz, px, py, pz);
    }
    cnt[l] = kept;
    if (cnt_own) cnt_own[l] = owns_cell(ob, ix, iy, iz) ? kept : 0;
}

// the points of the owned cells: slot off_own[l] + j of p (the arrays from the first new slot on), id = id0 + off[l] + j
__global__ __launch_bounds__(256) void k_src_emit(Grid g, Box box, SrcArgs a, OwnBox ob, SolidView sv, const int* __restrict__ hist,
                                                  const int* off, const int* off_own, Particles p, uint32_t id0, double vx, double vy, double vz)
{
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= box.cells()) return;
    int ix, iy, iz;
    const int m = src_tries(g.N, box, a, sv, hist, l, ix, iy, iz);
    if (m == 0 || !owns_cell(ob, ix, iy, iz)) return;
    const uint64_t h = src_cell_hash(g.N, a, ix, iy, iz);
    long j = off_own[l];
    uint32_t id = id0 + (uint32_t)off[l];
    for (int k = 0; k < m; ++k) {
        double px, py, pz;
        if (!src_point(h, k, g.lo + ix, g.lo + iy, g.lo + iz, px, py, pz)) continue;
        p.px[j] = px; p.py[j] = py; p.pz[j] = pz;
        p.vx[j] = vx; p.vy[j] = vy; p.vz[j] = vz;
        p.pid[j] = id++;
        ++j;
    }
}

// fluid_add_particles: host AoS -> the arrays after the live particles, pids pid0 + j
__global__ __launch_bounds__(256) void k_src_append(long n, const double* __restrict__ pos, const double* __restrict__ vel, Particles p, uint32_t pid0)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    p.px[j] = pos[3 * j]; p.py[j] = pos[3 * j + 1]; p.pz[j] = pos[3 * j + 2];
    if (vel) { p.vx[j] = vel[3 * j]; p.vy[j] = vel[3 * j + 1]; p.vz[j] = vel[3 * j + 2]; }
    else { p.vx[j] = 0; p.vy[j] = 0; p.vz[j] = 0; }
    p.pid[j] = pid0 + (uint32_t)j;
}

// ---- interpFromGrid (fluid.cc:883-894): v = clampedCatmullRom(p) over getVelocity(c, vels) (fluid.cc:58-70, 125-207) -----
// The same spline values, 3 x 3 x 3 cell order and association as k_g2p's PIC gather, but cells outside W are skipped
// rather than added with weight 0 (the reference's `if (isWithinBounds(.., 58))`).  The clamp to +-bound only removes cells
// that the W test removes too.  centre(gx, gy, gz, cu, cv, cw_): the centre velocity of the cell at coordinates (gx, gy, gz),
// or false to skip it.
template <typename F>
__device__ __forceinline__ void interp_gather(const Grid& g, long i, const Particles& p, F centre)
{
    const double cx = p.px[i], cy = p.py[i], cz = p.pz[i];
    const int wlo = g.lo + 2, whi = g.hi - 2;
    const int fcx = (int)round(cx), fcy = (int)round(cy), fcz = (int)round(cz);
    double wx[3], wy[3], wz[3];
    bool ix[3], iy[3], iz[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int ax = fcx - 1 + d, ay = fcy - 1 + d, az = fcz - 1 + d;
        ix[d] = ax >= wlo && ax <= whi;
        iy[d] = ay >= wlo && ay <= whi;
        iz[d] = az >= wlo && az <= whi;
        wx[d] = spline_at(cx, ax, d);
        wy[d] = spline_at(cy, ay, d);
        wz[d] = spline_at(cz, az, d);
    }
    double weight = 0, su = 0, sv = 0, sw = 0;
    for (int xi = 0; xi < 3; ++xi) {
        if (!ix[xi]) continue;
        for (int yi = 0; yi < 3; ++yi) {
            if (!iy[yi]) continue;
            for (int zi = 0; zi < 3; ++zi) {
                if (!iz[zi]) continue;
                double cu, cv, cw_;
                if (!centre(fcx - 1 + xi, fcy - 1 + yi, fcz - 1 + zi, cu, cv, cw_)) continue;
                const double cw = wx[xi] * wy[yi] * wz[zi];
                weight += cw;
                su += cu * cw;
                sv += cv * cw;
                sw += cw_ * cw;
            }
        }
    }
    if (weight != 0) {
        p.vx[i] = su / weight; p.vy[i] = sv / weight; p.vz[i] = sw / weight;
    } else {
        p.vx[i] = 0; p.vy[i] = 0; p.vz[i] = 0;
    }
}

// over full-size face arrays (origin 0): the cell velocities are the face averages formed here (k_g2p's pc* fields are left
// unallocated: allocating them would switch k_g2p to its blend branch).  Every cell read lies in W, its +1 faces on the grid.
__global__ __launch_bounds__(256) void k_interp_from_grid(Grid g, long n, Particles p, const double* __restrict__ u, const double* __restrict__ v,
                                                          const double* __restrict__ w)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long sx = g.sx(), sy = g.nz;
    interp_gather(g, i, p, [&](int gx, int gy, int gz, double& cu, double& cv, double& cw_) {
        const size_t c = g.idx(gx - g.lo, gy - g.lo, gz - g.lo);
        cu = (u[c] + u[c + sx]) / 2.0, cv = (v[c] + v[c + sy]) / 2.0, cw_ = (w[c] + w[c + 1]) / 2.0;
        return true;
    });
}

// ---- sinks ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_any_sink(const Grid& g, const SinkSet& sk, double x, double y, double z)
{
    bool gone = false;
    int lx, ly, lz;
    for (int b = 0; b < sk.n; ++b) gone = gone || in_box(g, sk.box[b], x, y, z, lx, ly, lz);
    return gone;
}
// *total += the threads of the block with `gone` set: a ballot and one atomic per wave (every thread of the block calls it)
template <typename T>
__device__ __forceinline__ void count_gone(bool gone, T* total)
{
    const unsigned long long m = __ballot(gone);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(total, (T)__popcll(m));
}

// One GPU: *removed += the particles whose base cell lies in a sink box.  keep_dev != nullptr (only once some are known to go):
// also keep_dev[i] (device order) and keep_pid[pid] (pid order) = 1 for the others, 0 for them
__global__ __launch_bounds__(256) void k_sink_mark(Grid g, long n, Particles p, SinkSet sk, int* __restrict__ keep_dev, int* __restrict__ keep_pid,
                                                   int* __restrict__ removed)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool gone = false;
    if (i < n) {
        gone = in_any_sink(g, sk, p.px[i], p.py[i], p.pz[i]);
        if (keep_dev) {   // launch-uniform
            keep_dev[i] = gone ? 0 : 1;
            keep_pid[p.pid[i]] = gone ? 0 : 1;
        }
    }
    if (removed) count_gone(gone, removed);   // launch-uniform
}

// stable compaction a -> b in device order; pids renumbered to their rank among the survivors in pid order
__global__ __launch_bounds__(256) void k_sink_compact(long n, Particles a, Particles b, const int* __restrict__ keep_dev, const int* __restrict__ dev_off,
                                                      const int* __restrict__ pid_new)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep_dev[i]) return;
    const long j = dev_off[i];
    b.px[j] = a.px[i]; b.py[j] = a.py[i]; b.pz[j] = a.pz[i];
    b.vx[j] = a.vx[i]; b.vy[j] = a.vy[i]; b.vz[j] = a.vz[i];
    b.pid[j] = (uint32_t)pid_new[a.pid[i]];
}

// A rank of a decomposed run: a live particle whose base cell lies in a sink box dies where it is (no compaction, no renumbering:
// G2P, advect, the routing and k_pack_live skip the dead, the next sort drops them); *removed += their number
__global__ __launch_bounds__(256) void k_sink_kill(Grid g, long n, Particles p, SinkSet sk, unsigned long long* __restrict__ removed)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool gone = false;
    if (i < n && p.pid[i] != PID_DEAD) {
        gone = in_any_sink(g, sk, p.px[i], p.py[i], p.pz[i]);
        if (gone) p.pid[i] = PID_DEAD;
    }
    count_gone(gone, removed);
}

// ---- grid velocities of a window (a rank of a decomposed run) -----------------------------------------------------------------
// getVelocity(c, vels) (fluid.cc:58-70) on the cells of `box` (window coordinates, inside W: the +1 faces are in the window):
// the expressions of k_interp_from_grid, stored so that a 1-wide halo of them can come from the neighbours (u, v, w carry a
// 1-wide halo only, and the centre of c+1 needs the face at c+2)
__global__ __launch_bounds__(256) void k_centre_avg(Grid g, Box box, const double* __restrict__ u, const double* __restrict__ v,
                                                    const double* __restrict__ w, double* __restrict__ cu, double* __restrict__ cv,
                                                    double* __restrict__ cw)
{
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= box.cells()) return;
    const int nz = box.nz(), ny = box.ny();
    const int iz = box.z0 + (int)(l % nz), iy = box.y0 + (int)((l / nz) % ny), ix = box.x0 + (int)(l / ((long)nz * ny));
    const size_t c = g.idx(ix, iy, iz);
    const long sx = g.sx(), sy = g.nz;
    cu[c] = (u[c] + u[c + sx]) / 2.0;
    cv[c] = (v[c] + v[c + sy]) / 2.0;
    cw[c] = (w[c] + w[c + 1]) / 2.0;
}

// the gather over those stored centres: the same cells, weights, order and association
__global__ __launch_bounds__(256) void k_interp_from_centres(Grid g, long n, Particles p, const double* __restrict__ ccu,
                                                             const double* __restrict__ ccv, const double* __restrict__ ccw)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    interp_gather(g, i, p, [&](int gx, int gy, int gz, double& cu, double& cv, double& cw_) {
        const int wxi = gx - g.cx0(), wyi = gy - g.cy0(), wzi = gz - g.cz0();
        if (wxi < 0 || wxi >= g.nx || wyi < 0 || wyi >= g.ny || wzi < 0 || wzi >= g.nz) return false;   // (never for a point of an owned cell)
        const size_t c = g.idx(wxi, wyi, wzi);
        cu = ccu[c], cv = ccv[c], cw_ = ccw[c];
        return true;
    });
}

static inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

void launch_src_count(hipStream_t st, Grid g, long n, Particles p, Box box, int* hist, bool skip_dead)
{
    if (n > 0) hipLaunchKernelGGL(k_src_count, dim3(nblk(n)), dim3(256), 0, st, g, n, p, box, hist, skip_dead ? 1 : 0);
}
void launch_src_plan(hipStream_t st, Grid g, Box box, uint64_t h0, int per_cell, bool fill, OwnBox ob, SolidView sv, const int* hist, int* cnt,
                     int* cnt_own)
{
    const SrcArgs a{h0, per_cell, fill ? 1 : 0};
    hipLaunchKernelGGL(k_src_plan, dim3(nblk(box.cells())), dim3(256), 0, st, g, box, a, ob, sv, hist, cnt, cnt_own);
}
void launch_src_emit(hipStream_t st, Grid g, Box box, uint64_t h0, int per_cell, bool fill, OwnBox ob, SolidView sv, const int* hist, const int* off,
                     const int* off_own, Particles p, uint32_t id0, const double vel[3])
{
    const SrcArgs a{h0, per_cell, fill ? 1 : 0};
    hipLaunchKernelGGL(k_src_emit, dim3(nblk(box.cells())), dim3(256), 0, st, g, box, a, ob, sv, hist, off, off_own, p, id0, vel[0], vel[1], vel[2]);
}
void launch_src_append(hipStream_t st, long n, const double* pos, const double* vel, Particles p, uint32_t pid0)
{
    if (n > 0) hipLaunchKernelGGL(k_src_append, dim3(nblk(n)), dim3(256), 0, st, n, pos, vel, p, pid0);
}
void launch_interp_from_grid(hipStream_t st, Grid g, long n, Particles p, const double* u, const double* v, const double* w)
{
    if (n > 0) hipLaunchKernelGGL(k_interp_from_grid, dim3(nblk(n)), dim3(256), 0, st, g, n, p, u, v, w);
}
void launch_sink_mark(hipStream_t st, Grid g, long n, Particles p, const SinkSet& sk, int* keep_dev, int* keep_pid, int* removed)
{
    if (n > 0) hipLaunchKernelGGL(k_sink_mark, dim3(nblk(n)), dim3(256), 0, st, g, n, p, sk, keep_dev, keep_pid, removed);
}
void launch_sink_compact(hipStream_t st, long n, Particles a, Particles b, const int* keep_dev, const int* dev_off, const int* pid_new)
{
    if (n > 0) hipLaunchKernelGGL(k_sink_compact, dim3(nblk(n)), dim3(256), 0, st, n, a, b, keep_dev, dev_off, pid_new);
}
void launch_sink_kill(hipStream_t st, Grid g, long n, Particles p, const SinkSet& sk, unsigned long long* removed)
{
    if (n > 0) hipLaunchKernelGGL(k_sink_kill, dim3(nblk(n)), dim3(256), 0, st, g, n, p, sk, removed);
}
void launch_centre_avg(hipStream_t st, Grid g, Box box, const double* u, const double* v, const double* w, double* cu, double* cv, double* cw)
{
    if (box.cells() > 0) hipLaunchKernelGGL(k_centre_avg, dim3(nblk(box.cells())), dim3(256), 0, st, g, box, u, v, w, cu, cv, cw);
}
void launch_interp_from_centres(hipStream_t st, Grid g, long n, Particles p, const double* cu, const double* cv, const double* cw)
{
    if (n > 0) hipLaunchKernelGGL(k_interp_from_centres, dim3(nblk(n)), dim3(256), 0, st, g, n, p, cu, cv, cw);
}

}  // namespace fl
