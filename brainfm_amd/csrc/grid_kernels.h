// What the voxel-wise interpol grid kernels (spline_grid.hip, spline_grid2d.hip, grid_hess.hip, label_pull.hip) and their
// exports share: the launch shape, the options a call carries, the prologue of a voxel (of a pixel on a 2-D grid), the
// argument checks and the dispatch from the orders of a call to the instantiation that runs it.  The nodes themselves
// are axis_node / axis_nodes of spline_nodes.h.
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

// Voxel i of B * nvox: its batch, its index within the batch, its coordinate and the inbounds mask against (nx, ny, nz).
// The coordinate is three 4-byte ld_tex loads (gather3d.h: agent scope, and no wider load -- HISTORY.md section 3.3).
struct GridVoxel { int b; int64_t v; float gx, gy, gz, mask; };

__device__ __forceinline__ GridVoxel grid_voxel(int64_t i, int64_t nvox, const float* grid, int Bg, int nx,
                                                int ny, int nz, int extrap) {
    GridVoxel p;
    p.b = (int)(i / nvox);
    p.v = i - (int64_t)p.b * nvox;
    const float* g = grid + ((int64_t)(Bg == 1 ? 0 : p.b) * nvox + p.v) * 3;
    p.gx = ld_tex(g); p.gy = ld_tex(g + 1); p.gz = ld_tex(g + 2);
    p.mask = inbounds(p.gx, p.gy, p.gz, nx, ny, nz, extrap);
    return p;
}

// Pixel i of B * npix of a 2-D grid [Bg][*out][2] against (nx, ny): two ld_tex loads and the 2-D mask
struct GridPixel { int b; int64_t v; float gx, gy, mask; };

__device__ __forceinline__ GridPixel grid_pixel(int64_t i, int64_t npix, const float* grid, int Bg, int nx, int ny,
                                                int extrap) {
    GridPixel p;
    p.b = (int)(i / npix);
    p.v = i - (int64_t)p.b * npix;
    const float* g = grid + ((int64_t)(Bg == 1 ? 0 : p.b) * npix + p.v) * 2;
    p.gx = ld_tex(g); p.gy = ld_tex(g + 1);
    p.mask = inbounds(p.gx, p.gy, nx, ny, extrap);
    return p;
}

// the argument checks of the _linear exports (synth_interp.hip) plus the orders; (a0, a1, a2) and (b0, b1, b2) are the two
// spatial shapes of the call
inline int grid_check_args(const void* inp, const void* grid, const void* out, const int* bound, const int* order, int Bi,
                           int Bg, int C, int a0, int a1, int a2, int b0, int b1, int b2, int extrapolate) {
    if (!inp || !grid || !out || !bound || !order || Bi <= 0 || Bg <= 0 || C <= 0 || a0 <= 0 || a1 <= 0 || a2 <= 0 ||
        b0 <= 0 || b1 <= 0 || b2 <= 0)
        return BFM_E_ARG;
    if (Bi != Bg && Bi != 1 && Bg != 1) return BFM_E_SHAPE;
    for (int a = 0; a < 3; ++a) if (bound[a] < 0 || bound[a] > 6) return BFM_E_ARG;
    for (int a = 0; a < 3; ++a) if (order[a] < 0 || order[a] > 3) return BFM_E_ARG;
    if (extrapolate < 0 || extrapolate > 2) return BFM_E_ARG;
    return BFM_OK;
}

inline GridOpts grid_opts(const int* bound, const int* order, int extrapolate) {
    return GridOpts{extrapolate, {bound[0], bound[1], bound[2]}, {order[0], order[1], order[2]}};
}

// The 2-D exports read bound[2] and order[2]: the same checks over two axes and two extents per shape (a 3-D call with a
// third extent of 1, bound 0 and the order of the second axis, which keeps an isotropic 2-D call isotropic), and the
// options with that third axis, which no 2-D kernel reads.
inline int grid_check_args(const void* inp, const void* grid, const void* out, const int* bound, const int* order, int Bi,
                           int Bg, int C, int a0, int a1, int b0, int b1, int extrapolate) {
    if (!bound || !order) return BFM_E_ARG;
    const int b3[3] = {bound[0], bound[1], 0}, o3[3] = {order[0], order[1], order[1]};
    return grid_check_args(inp, grid, out, b3, o3, Bi, Bg, C, a0, a1, 1, b0, b1, 1, extrapolate);
}

inline GridOpts grid_opts2(const int* bound, const int* order, int extrapolate) {
    return GridOpts{extrapolate, {bound[0], bound[1], 0}, {order[0], order[1], order[1]}};
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
