// What the point-wise interpol grid kernels (spline_grid.hip, grid_hess.hip, label_pull.hip) and their exports share, for
// 2-D and 3-D grids alike: the launch shape, the options a call carries, the prologue of a grid point, the argument
// checks and the dispatch from the orders of a call to the instantiation that runs it.  The nodes themselves are
// axis_node / axis_nodes of spline_nodes.h.
//
// One thread per voxel of the grid (the output of pull / grad / hess, the source of push / pushgrad).  A kernel is
// instantiated for some isotropic orders O with O + 1 taps per axis, so that every array is indexed by constants and
// nothing goes to scratch, and once with O = -1 for every other combination: per-axis orders from the options and 4 taps
// per axis, where an unused tap has weight 0 and the index of tap 0.
#pragma once
#include <type_traits>

#include "bfm_common.h"
#include "gather3d.h"
#include "interp_bounds.h"
#include "spline_nodes.h"

inline int grid_for(int64_t n, int tpb = 256, int cap = 8192) {
    int64_t b = bfm_cdiv64(n, tpb);
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

#define GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// extrapolate (0 no / 1 yes / 2 hist) and the bounds and orders per axis, passed to the kernels by value.  extrap stands in
// front of the bounds on purpose: behind the orders it is fetched apart from them, and label_pull3d_regs<2> then comes
// out 5 % longer and 11 % slower at the same register count (profiles/grid_family_refactor.txt).
struct GridOpts { int extrap; int bound[3]; int order[3]; };

constexpr int grid_taps(int O) { return O < 0 ? 4 : O + 1; }

// the order of axis a under instantiation O
template <int O>
__device__ __forceinline__ int axis_order(const GridOpts& op, int a) { return O < 0 ? op.order[a] : O; }

// the D spatial extents of an image, passed to the kernels by value
template <int D>
struct GridDims {
    int n[D];
    __host__ __device__ int64_t count() const {
        int64_t c = 1;
        for (int a = 0; a < D; ++a) c *= n[a];
        return c;
    }
};

// Point i of B * npts of a grid [Bg][*out][D]: its batch, its index within the batch, its coordinate and the inbounds mask
// against `dims`.  The coordinate is D 4-byte ld_tex loads (gather3d.h: agent scope, and no wider load -- HISTORY.md
// section 3.3).
template <int D>
struct GridPoint { int b; int64_t v; float g[D]; float mask; };

template <int D>
__device__ __forceinline__ GridPoint<D> grid_point(int64_t i, int64_t npts, const float* grid, int Bg, const GridDims<D>& dims,
                                                   int extrap) {
    GridPoint<D> p;
    p.b = (int)(i / npts);
    p.v = i - (int64_t)p.b * npts;
    const float* g = grid + ((int64_t)(Bg == 1 ? 0 : p.b) * npts + p.v) * D;
#pragma unroll
    for (int a = 0; a < D; ++a) p.g[a] = ld_tex(g + a);
    p.mask = inbounds<D>(p.g, dims.n, extrap);
    return p;
}

// the orders an all-linear export, which takes none from its caller, hands to the checks and the options
constexpr int GRID_LINEAR[3] = {1, 1, 1};

// The argument checks of every export of the family; a and b are the two spatial shapes of the call, D extents each, and
// the first D bounds and orders are read.  The _linear exports, which take no orders, pass GRID_LINEAR.
inline int grid_check_args(int D, const void* inp, const void* grid, const void* out, const int* bound, const int* order,
                           int Bi, int Bg, int C, const int* a, const int* b, int extrapolate) {
    if (!inp || !grid || !out || !bound || !order || Bi <= 0 || Bg <= 0 || C <= 0) return BFM_E_ARG;
    for (int k = 0; k < D; ++k) if (a[k] <= 0 || b[k] <= 0) return BFM_E_ARG;
    if (Bi != Bg && Bi != 1 && Bg != 1) return BFM_E_SHAPE;
    for (int k = 0; k < D; ++k) if (bound[k] < 0 || bound[k] > 6) return BFM_E_ARG;
    for (int k = 0; k < D; ++k) if (order[k] < 0 || order[k] > 3) return BFM_E_ARG;
    if (extrapolate < 0 || extrapolate > 2) return BFM_E_ARG;
    return BFM_OK;
}

// The options of a call on D axes.  An axis beyond D, which no kernel of that dimension reads, takes bound 0 and the order
// of the last axis, so that an isotropic 2-D call stays isotropic for dispatch_order.
inline GridOpts grid_opts(int D, const int* bound, const int* order, int extrapolate) {
    GridOpts op{extrapolate, {0, 0, 0}, {0, 0, 0}};
    for (int k = 0; k < 3; ++k) {
        if (k < D) op.bound[k] = bound[k];
        op.order[k] = order[k < D ? k : D - 1];
    }
    return op;
}

// the order of an isotropic call, -1 for any other
inline int iso_order(const int* o) { return (o[0] == o[1] && o[1] == o[2]) ? o[0] : -1; }

// f(std::integral_constant<int, O>) for the O of Os... that the call's orders are isotropic in, and for O = -1 (the padded
// instantiation) when there is none: Os are the orders a kernel has its own instantiation for.
template <int... Os, typename F>
inline void dispatch_order(const int* order, F&& f) {
    const int iso = iso_order(order);
    if (!((iso == Os ? (f(std::integral_constant<int, Os>{}), true) : false) || ...)) f(std::integral_constant<int, -1>{});
}
