// ORACLE — TEST INFRASTRUCTURE ONLY (builds into oracle/_ref/, git-ignored).
//
// OpenVDB's own level-set operators over a mock dense grid, compiled from the lines the Makefile takes out of the reference tree ($(REF)) at
// build time (nothing of the reference is committed, the extracts are deleted after the compile).  math/Math.h, math/Vec3.h and
// math/Coord.h are included whole, against the two stand-in headers of oracle/shim/boost.  Taken as they are:
//   math/FiniteDifference.h   59-77, 177-184, 192-201 (scheme enums), 261-268 (TemporalIntegrationScheme), 329-374 (WENO5,
//                             GodunovsNormSqrd), 384-392, 463-486, 541-597, 747-797 (D1: CD_2ND, FD_1ST, BD_1ST), 938-989,
//                             1223-1320, 1427-1530 (D1: FD / BD HJWENO5), 1809-1963 (D2<CD_SECOND>)
//   math/Stencils.h           55-1688 (every stencil; BaseStencil::median is the median filter's selection, run here over the
//                             DenseStencil as the filter does and over the eight-point BoxStencil, for the rank of an even count)
//   math/Operators.h          121-216 (ISGradient, BIAS_SCHEME), 252-284 (ISGradientNormSqrd), 369-404, 554-631
//   tools/LevelSetTracker.h   489-491 (mDt, mInvDx) into the initialiser list of Normalizer below; 599-608 (the body of
//                             Normalizer::eval) into the body of Normalizer::eval below; 625 (the stencil) and 632-633 (move the
//                             stencil, call eval) into Normalizer::euler below
//   tools/LevelSetFilter.h    212-226 (Avg), 231-233 (boxX / boxY / boxZ), 303-310 (the three passes of box()),
//                             358-365 (the offset's stepping, up to the task it binds and cooks); per pass the time step, the
//                             stencil or average, and the update of a voxel: 384, 385, 404-405 (mean curvature), 425, 426, 445-446
//                             (Laplacian), 484, 502-503 (median), 517, 533 (box)
// Ours, and only so: the mock grid (DenseTree, tree::ValueAccessor, DenseGrid, VoxelIt), the mock parent of the filter and of the
// tracker (voxelSize(), grid(), checkInterrupter()), boost::bind / _1 / _2 / cook() reduced to "call the bound member now",
// box<AvgT>() and offset(range, value), which only record what they were called with, for_active(): the walk over the active voxels
// in C order with the inactive ones copied into the output first (the reference walks leaves and their on-voxels and writes the
// leaf's second buffer), the BoxStencil of medianOfEightPass, and the extern "C" surface.  Every statement that reads or writes a
// voxel's value inside those walks is an extracted line.
#include <openvdb/math/Math.h>
#include <openvdb/math/Vec3.h>
#include <openvdb/math/Coord.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

// ---- boost::bind as the filter uses it: (member, _1, _2[, argument]) -> callable(object, range) -------------------------------
struct VdbRefPlaceholder {};
static const VdbRefPlaceholder _1 = {}, _2 = {};
namespace boost {
template<typename C, typename R, typename A, typename V>
std::function<void(C*, const R&)> bind(void (C::*f)(const R&, A), VdbRefPlaceholder, VdbRefPlaceholder, V a)
{
    const A arg = static_cast<A>(a);
    return [f, arg](C* self, const R& r) { (self->*f)(r, arg); };
}
}  // namespace boost

namespace openvdb {
OPENVDB_USE_VERSION_NAMESPACE
namespace OPENVDB_VERSION_NAME {

typedef double Real;
typedef uint32_t Index;
typedef int32_t Int32;
using math::Coord;

// ---- the mock grid: a dense (n, n, n) C-order array, the background outside it ------------------------------------------------
struct DenseTree {
    typedef float ValueType;
    const float* v;
    int n;
    float bg;
    float get(const Coord& c) const
    {
        const int i = c[0], j = c[1], k = c[2];
        if (i < 0 || j < 0 || k < 0 || i >= n || j >= n || k >= n) return bg;
        return v[(size_t(i) * n + j) * n + k];
    }
};
namespace tree {
template<typename TreeT, bool IsSafe>
struct ValueAccessor {
    typedef typename TreeT::ValueType ValueType;
    explicit ValueAccessor(TreeT& t): mTree(&t) {}
    ValueType getValue(const Coord& c) const { return mTree->get(c); }
    TreeT* mTree;
};
}  // namespace tree
struct DenseGrid {
    typedef DenseTree TreeType;
    typedef float ValueType;
    typedef tree::ValueAccessor<const DenseTree, true> ConstAccessor;
    DenseTree t;
    double dx;
    const TreeType& tree() const { return t; }
    math::Vec3<double> voxelSize() const { return math::Vec3<double>(dx, dx, dx); }
    float background() const { return t.bg; }
};
struct VoxelIt {   // what the stencils' moveTo(iter) and the passes read of a leaf's voxel iterator; pos() indexes the dense array
    Coord c;
    float v;
    Index p;
    Coord getCoord() const { return c; }
    float operator*() const { return v; }
    Index pos() const { return p; }
};

// every active voxel in C order: f(iterator); inactive voxels keep their value
template<typename Fn>
void for_active(const float* val, const uint8_t* act, int n, float* out, Fn f)
{
    std::memcpy(out, val, sizeof(float) * size_t(n) * n * n);
    Index idx = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < n; ++k, ++idx)
                if (act[idx]) f(VoxelIt{Coord(i, j, k), val[idx], idx});
}

namespace math {
#include "_ref/vdb_fd_extract.inc"
#include "_ref/vdb_stencils_extract.inc"
#include "_ref/vdb_operators_extract.inc"
}  // namespace math

namespace tools {

struct MockTracker {   // LevelSetTracker::voxelSize() is the grid's, narrowed to ValueType (tools/LevelSetTracker.h:175, 259)
    float dx;
    const DenseGrid* g;
    float voxelSize() const { return dx; }
    const DenseGrid& grid() const { return *g; }
};

template<math::BiasedGradientScheme SpatialScheme, math::TemporalIntegrationScheme TemporalScheme>
struct Normalizer {
    typedef DenseGrid::ValueType ValueType;
    typedef typename math::BIAS_SCHEME<SpatialScheme>::template ISStencil<DenseGrid>::StencilType StencilT;
    explicit Normalizer(MockTracker& tracker)
        : mTracker(tracker)
#include "_ref/vdb_tracker_dt_extract.inc"
    {
    }
    template<int Nominator, int Denominator>
    void eval(StencilT& stencil, const ValueType* phi, ValueType* result, Index n) const
    {
#include "_ref/vdb_tracker_eval_extract.inc"
    }
    // one Euler step over the active voxels (tools/LevelSetTracker.h:619-644 without the mask); phi and result are the leaf buffers
    template<int Nominator, int Denominator>
    void euler(const ValueType* phi, const uint8_t* act, int n, ValueType* result)
    {
#include "_ref/vdb_tracker_stencil_extract.inc"
        for_active(phi, act, n, result, [&](const VoxelIt& iter) {
#include "_ref/vdb_tracker_step_extract.inc"
        });
    }
    MockTracker& mTracker;
    const ValueType mDt, mInvDx;
};

struct LeafRange {};

struct Filter {
    typedef DenseGrid GridT;
    typedef DenseGrid GridType;
    typedef DenseGrid::ValueType ValueType;
    struct Parent {
        ValueType dx;
        const GridT* g;
        ValueType voxelSize() const { return dx; }
        bool checkInterrupter() const { return true; }
        const GridT& grid() const { return *g; }
    };

#include "_ref/vdb_filter_avg_extract.inc"

    template<typename AvgT>
    void box(const LeafRange& r, Int32 w);   // records AvgT's axis

#include "_ref/vdb_filter_boxnames_extract.inc"

    void boxPasses(int width)
    {
#include "_ref/vdb_filter_boxorder_extract.inc"
    }

    void cook(bool) { mTask(this, LeafRange()); }
    void offset(const LeafRange&, ValueType v) { mSteps.push_back(v); }   // records the step a pass would add

    void offsetSteps(ValueType value)
    {
#include "_ref/vdb_filter_offset_extract.inc"
        }
    }
    // the four passes over the active voxels: the stencil (or the average) and the update are the reference's lines, `buffer` is the
    // leaf's second buffer (tools/LevelSetFilter.h:391, 432, 490, 523), here the output array
    void meanCurvaturePass(const ValueType* val, const uint8_t* act, int n, ValueType* buffer)
    {
#include "_ref/vdb_filter_dtcurv_extract.inc"
#include "_ref/vdb_filter_curvstencil_extract.inc"
        for_active(val, act, n, buffer, [&](const VoxelIt& iter) {
#include "_ref/vdb_filter_curvstep_extract.inc"
        });
    }
    void laplacianPass(const ValueType* val, const uint8_t* act, int n, ValueType* buffer)
    {
#include "_ref/vdb_filter_dtlap_extract.inc"
#include "_ref/vdb_filter_lapstencil_extract.inc"
        for_active(val, act, n, buffer, [&](const VoxelIt& iter) {
#include "_ref/vdb_filter_lapstep_extract.inc"
        });
    }
    void medianPass(const ValueType* val, const uint8_t* act, int n, ValueType* buffer, int width)
    {
#include "_ref/vdb_filter_medstencil_extract.inc"
        for_active(val, act, n, buffer, [&](const VoxelIt& iter) {
#include "_ref/vdb_filter_medstep_extract.inc"
        });
    }
    // BaseStencil::median() over a stencil of even size, the eight values of the BoxStencil at (i..i+1, j..j+1, k..k+1): no filter
    // runs it, it shows which of the two middle ranks the selection takes.  The stencil is ours, the two lines are the median pass's
    void medianOfEightPass(const ValueType* val, const uint8_t* act, int n, ValueType* buffer)
    {
        math::BoxStencil<GridType> stencil(mParent->grid());
        for_active(val, act, n, buffer, [&](const VoxelIt& iter) {
#include "_ref/vdb_filter_medstep_extract.inc"
        });
    }
    template<typename AvgT>
    void boxPass(const ValueType* val, const uint8_t* act, int n, ValueType* buffer, Int32 w)
    {
#include "_ref/vdb_filter_avgof_extract.inc"
        for_active(val, act, n, buffer, [&](const VoxelIt& iter) {
#include "_ref/vdb_filter_boxstep_extract.inc"
        });
    }

    ValueType dtCurvature() const
    {
#include "_ref/vdb_filter_dtcurv_extract.inc"
        return dt;
    }
    ValueType dtLaplacian() const
    {
#include "_ref/vdb_filter_dtlap_extract.inc"
        return dt;
    }

    Parent parent;
    Parent* mParent;
    std::function<void(Filter*, const LeafRange&)> mTask;
    std::vector<int> mAxes;
    std::vector<ValueType> mSteps;

    Filter(ValueType dx, const GridT* g): parent{dx, g}, mParent(&parent) {}
};

template<typename T> struct AxisOf;
template<size_t A> struct AxisOf<Filter::Avg<A> > { enum { value = int(A) }; };

template<typename AvgT>
void Filter::box(const LeafRange&, Int32) { mAxes.push_back(AxisOf<AvgT>::value); }

}  // namespace tools
}  // namespace OPENVDB_VERSION_NAME
}  // namespace openvdb

namespace {
using namespace openvdb;

DenseGrid grid_of(const float* val, int n, float bg, float dx)
{
    DenseGrid g;
    g.t.v = val;
    g.t.n = n;
    g.t.bg = bg;
    g.dx = double(dx);
    return g;
}

template<math::BiasedGradientScheme S>
void normalize(const float* val, const uint8_t* act, int n, float bg, float dx, float* out)
{
    typedef tools::Normalizer<S, math::TVD_RK1> N;
    const DenseGrid g = grid_of(val, n, bg, dx);
    tools::MockTracker tracker{dx, &g};
    N norm(tracker);
    norm.template euler<0, 1>(val, act, n, out);   // euler01 (tools/LevelSetTracker.h:221): TVD_RK1's one step
}

template<math::BiasedGradientScheme S>
void voxel(const float* ux, const float* uy, const float* uz, long count, float dx, float* out)
{
    // a 7^3 grid whose three axis lines through the centre hold the septuples; the stencils of both schemes read nothing else
    typedef tools::Normalizer<S, math::TVD_RK1> N;
    std::vector<float> cube(343, 0.0f), res(343);
    std::vector<uint8_t> centre(343, 0);
    centre[171] = 1;
    const DenseGrid g = grid_of(cube.data(), 7, 0.0f, dx);
    tools::MockTracker tracker{dx, &g};
    N norm(tracker);
    for (long c = 0; c < count; ++c) {
        for (int k = 0; k < 7; ++k) {
            cube[(k * 7 + 3) * 7 + 3] = ux[k * count + c];
            cube[(3 * 7 + k) * 7 + 3] = uy[k * count + c];
            cube[(3 * 7 + 3) * 7 + k] = uz[k * count + c];
        }
        norm.template euler<0, 1>(cube.data(), centre.data(), 7, res.data());
        out[c] = res[171];
    }
}
}  // namespace

extern "C" {

int vdb_ref_normalize(const float* val, const uint8_t* act, int n, float bg, float dx, int scheme, float* out)
{
    if (scheme == int(math::FIRST_BIAS)) normalize<math::FIRST_BIAS>(val, act, n, bg, dx, out);
    else if (scheme == int(math::HJWENO5_BIAS)) normalize<math::HJWENO5_BIAS>(val, act, n, bg, dx, out);
    else return -1;
    return 0;
}

void vdb_ref_laplacian(const float* val, const uint8_t* act, int n, float bg, float dx, float* out)
{
    const DenseGrid g = grid_of(val, n, bg, dx);
    tools::Filter f(dx, &g);
    f.laplacianPass(val, act, n, out);
}

void vdb_ref_curvature(const float* val, const uint8_t* act, int n, float bg, float dx, float* out)
{
    const DenseGrid g = grid_of(val, n, bg, dx);
    tools::Filter f(dx, &g);
    f.meanCurvaturePass(val, act, n, out);
}

void vdb_ref_median(const float* val, const uint8_t* act, int n, float bg, int width, float* out)
{
    const DenseGrid g = grid_of(val, n, bg, 1.0f);
    tools::Filter f(1.0f, &g);
    f.medianPass(val, act, n, out, width);
}

void vdb_ref_median_of_eight(const float* val, const uint8_t* act, int n, float bg, float* out)
{
    const DenseGrid g = grid_of(val, n, bg, 1.0f);
    tools::Filter f(1.0f, &g);
    f.medianOfEightPass(val, act, n, out);
}

int vdb_ref_box(const float* val, const uint8_t* act, int n, float bg, int axis, int width, float* out)
{
    const DenseGrid g = grid_of(val, n, bg, 1.0f);
    tools::Filter f(1.0f, &g);
    if (axis == 0) f.boxPass<tools::Filter::Avg<0> >(val, act, n, out, width);
    else if (axis == 1) f.boxPass<tools::Filter::Avg<1> >(val, act, n, out, width);
    else if (axis == 2) f.boxPass<tools::Filter::Avg<2> >(val, act, n, out, width);
    else return -1;
    return 0;
}

// passes[3]: the axis of the first, second and third pass of box(); names[3]: the axis boxX, boxY and boxZ average along
void vdb_ref_box_order(int* passes, int* names)
{
    tools::Filter f(1.0f, nullptr);
    f.boxPasses(1);
    for (int i = 0; i < 3; ++i) passes[i] = i < int(f.mAxes.size()) ? f.mAxes[i] : -1;
    if (f.mAxes.size() != 3) passes[0] = -1;
    tools::Filter h(1.0f, nullptr);
    h.boxX(tools::LeafRange(), 1);
    h.boxY(tools::LeafRange(), 1);
    h.boxZ(tools::LeafRange(), 1);
    for (int i = 0; i < 3; ++i) names[i] = h.mAxes[i];
}

int vdb_ref_offset_steps(float value, float dx, float* out, int cap)
{
    tools::Filter f(dx, nullptr);
    f.offsetSteps(value);
    const int m = int(f.mSteps.size());
    for (int i = 0; i < m && i < cap; ++i) out[i] = f.mSteps[i];
    return m;
}

// out[4]: the normaliser's dt and 1/dx, the Laplacian flow's dt, the curvature flow's dt
void vdb_ref_consts(float dx, float* out)
{
    tools::MockTracker tracker{dx, nullptr};
    const tools::Normalizer<math::FIRST_BIAS, math::TVD_RK1> norm(tracker);
    tools::Filter f(dx, nullptr);
    out[0] = norm.mDt;
    out[1] = norm.mInvDx;
    out[2] = f.dtLaplacian();
    out[3] = f.dtCurvature();
}

void vdb_ref_weno5(const float* v1, const float* v2, const float* v3, const float* v4, const float* v5, long count, float* out)
{
    for (long c = 0; c < count; ++c) out[c] = math::WENO5<float>(v1[c], v2[c], v3[c], v4[c], v5[c]);
}

// u is (7, count): u[k + 3] = val(c + k e); dm / dp are D1<BD_HJWENO5> / D1<FD_HJWENO5>::difference in the stencil versions' order
void vdb_ref_axis_diffs(const float* u, long count, float* dm, float* dp)
{
    for (long c = 0; c < count; ++c) {
        float s[7];
        for (int k = 0; k < 7; ++k) s[k] = u[k * count + c];
        dp[c] = math::D1<math::FD_HJWENO5>::difference(s[6], s[5], s[4], s[3], s[2], s[1]);
        dm[c] = math::D1<math::BD_HJWENO5>::difference(s[0], s[1], s[2], s[3], s[4], s[5]);
    }
}

int vdb_ref_voxel(const float* ux, const float* uy, const float* uz, long count, float dx, int scheme, float* out)
{
    if (scheme == int(math::FIRST_BIAS)) voxel<math::FIRST_BIAS>(ux, uy, uz, count, dx, out);
    else if (scheme == int(math::HJWENO5_BIAS)) voxel<math::HJWENO5_BIAS>(ux, uy, uz, count, dx, out);
    else return -1;
    return 0;
}
}
