// interpol grid_pull / grid_push / grid_grad on 2-D grids for spline orders 0 to 3, any order per axis: what the vendored
// torch-interpol computes in iso0.pull2d / push2d (iso0.py), iso1.pull2d / push2d / grad2d (iso1.py) and, for every other
// combination of orders, the generic path (utils/interpol/nd.py:30-290, splines.py:30-43 and :90-103, bounds.py:24-89).
//
// Layouts: image [B][C][nx][ny], grid [Bg][*out][2], gradient [B][C][nout][2].  One thread per grid pixel (the output of
// pull / grad, the source of push).  Nodes, signs and weights come from axis_nodes (spline_nodes.h), once per pixel into
// registers with the sign folded into the weight; the channel loop is inside.  Every texel and coordinate load is ld_tex
// (gather3d.h).  The isotropic orders 0, 1, 2 and 3 are instantiated with their tap counts (1, 2, 3, 4 per axis), so
// every array is indexed by constants and nothing goes to scratch; a mixed-order call runs the instantiation padded to
// 4 x 4 taps, where an unused tap has weight 0 and the index of tap 0.  The pixel prologue, the options struct, the
// argument checks and the dispatch are grid_kernels.h, shared with the 3-D kernels.
//
// 2-D has no separate linear kernels: order {1,1} is an instantiation here.  Its gradient takes the slope of iso1.grad2d
// (-1 at the lower node, +1 at the upper), which is what the reference runs for an all-linear call; a linear axis of a
// mixed-order call takes the generic path's sign(x) (splines.py:93-97), the opposite sign, as in 3-D.
//
// The sums are (wx * wy) * value accumulated tap by tap, x outer and y inner, the mask last: the terms and the order of
// spline_pull3d on the image [nx][ny][1] with a third coordinate 0 and order 0 on the third axis, whose extra factor is an
// exact 1 and whose padded taps add exact zeros.
#include "grid_kernels.h"

namespace {

// O = 0..3: isotropic order O with O + 1 taps per axis; O < 0: per-axis orders from `op`, 4 taps per axis
template <int O>
__global__ void __launch_bounds__(256) spline_pull2d(const float* __restrict__ inp, int Bi, int C, int nx, int ny,
                                                     const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op,
                                                     int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1);
    const int64_t n = (int64_t)B * nout;
    const int64_t area = (int64_t)nx * ny;
    GRID_STRIDE(i, n) {
        const GridPixel p = grid_pixel(i, nout, grid, Bg, nx, ny, op.extrap);
        int ix[T], iy[T];
        float wx[T], wy[T];
        axis_nodes<T>(p.gx, ox, nx, op.bound[0], ix, wx);
        axis_nodes<T>(p.gy, oy, ny, op.bound[1], iy, wy);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * area;
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < T; ++a) {
                const float* row = src + (int64_t)ix[a] * ny;
#pragma unroll
                for (int bb = 0; bb < T; ++bb) acc = fmaf(ld_tex(row + iy[bb]), wx[a] * wy[bb], acc);
            }
            out[((int64_t)p.b * C + c) * nout + p.v] = acc * p.mask;
        }
    }
}

// The adjoint of pull: every source pixel scatters its value to its nodes.  out [B][C][nx*ny] must be zero on entry.  fp32
// atomics, so the summation order, and with it the last bit, is not reproducible.  A tap whose weight times sign is exactly
// 0 (a node the `zero` bound drops, a padded tap) issues nothing, and neither does a masked pixel.
template <int O>
__global__ void __launch_bounds__(256) spline_push2d(const float* __restrict__ inp, int Bi, int C,
                                                     const float* __restrict__ grid, int Bg, int64_t nin, int nx, int ny,
                                                     GridOpts op, int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1);
    const int64_t n = (int64_t)B * nin;
    const int64_t area = (int64_t)nx * ny;
    GRID_STRIDE(i, n) {
        const GridPixel p = grid_pixel(i, nin, grid, Bg, nx, ny, op.extrap);
        if (p.mask == 0.f) continue;
        int ix[T], iy[T];
        float wx[T], wy[T];
        axis_nodes<T>(p.gx, ox, nx, op.bound[0], ix, wx);
        axis_nodes<T>(p.gy, oy, ny, op.bound[1], iy, wy);
        for (int c = 0; c < C; ++c) {
            const float val = inp[((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * nin + p.v];
            float* dst = out + ((int64_t)p.b * C + c) * area;
#pragma unroll
            for (int a = 0; a < T; ++a) {
                float* row = dst + (int64_t)ix[a] * ny;
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const float w = wx[a] * wy[bb];
                    if (w != 0.f) atomicAdd(row + iy[bb], val * w);
                }
            }
        }
    }
}

// out [B][C][nout][2]; component d takes the derivative on axis d and the plain weight on the other.  O == 1: iso1's slope.
template <int O>
__global__ void __launch_bounds__(256) spline_grad2d(const float* __restrict__ inp, int Bi, int C, int nx, int ny,
                                                     const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op,
                                                     int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    constexpr bool ISO1 = O == 1;
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1);
    const int64_t n = (int64_t)B * nout;
    const int64_t area = (int64_t)nx * ny;
    GRID_STRIDE(i, n) {
        const GridPixel p = grid_pixel(i, nout, grid, Bg, nx, ny, op.extrap);
        int ix[T], iy[T];
        float wx[T], wy[T], dx[T], dy[T];
        axis_nodes<T, 1, ISO1>(p.gx, ox, nx, op.bound[0], ix, wx, dx);
        axis_nodes<T, 1, ISO1>(p.gy, oy, ny, op.bound[1], iy, wy, dy);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * area;
            float ax = 0.f, ay = 0.f;
#pragma unroll
            for (int a = 0; a < T; ++a) {
                const float* row = src + (int64_t)ix[a] * ny;
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const float val = ld_tex(row + iy[bb]);
                    ax = fmaf(val, dx[a] * wy[bb], ax);
                    ay = fmaf(val, wx[a] * dy[bb], ay);
                }
            }
            float* o = out + (((int64_t)p.b * C + c) * nout + p.v) * 2;
            o[0] = ax * p.mask; o[1] = ay * p.mask;
        }
    }
}

}  // namespace

// every isotropic order has its own instantiation; a mixed-order call runs the padded one
template <typename F>
static int launch_spline2d(const GridOpts& op, int64_t n, F&& launch) {
    dispatch_order<0, 1, 2, 3>(op.order, [&](auto o) { launch(o, dim3(grid_for(n)), dim3(256)); });
    return bfm_launch_status();
}

extern "C" int bfm_grid_pull2d_spline(const float* inp, int Bi, int C, int nx, int ny, const float* grid, int Bg, int ox,
                                      int oy, const int* bound, const int* order, int extrapolate, float* out,
                                      bfm_stream_t stream) {
    const int rc = grid_check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, ox, oy, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy;
    const GridOpts op = grid_opts2(bound, order, extrapolate);
    return launch_spline2d(op, B * nout, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_pull2d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, nx, ny, grid, Bg, nout,
                           op, B, out);
    });
}

extern "C" int bfm_grid_push2d_spline(const float* inp, int Bi, int C, int ix, int iy, const float* grid, int Bg, int nx,
                                      int ny, const int* bound, const int* order, int extrapolate, float* out_zeroed,
                                      bfm_stream_t stream) {
    const int rc = grid_check_args(inp, grid, out_zeroed, bound, order, Bi, Bg, C, ix, iy, nx, ny, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = (int64_t)ix * iy;
    const GridOpts op = grid_opts2(bound, order, extrapolate);
    return launch_spline2d(op, B * nin, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_push2d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, grid, Bg, nin, nx, ny,
                           op, B, out_zeroed);
    });
}

extern "C" int bfm_grid_grad2d_spline(const float* inp, int Bi, int C, int nx, int ny, const float* grid, int Bg, int ox,
                                      int oy, const int* bound, const int* order, int extrapolate, float* out,
                                      bfm_stream_t stream) {
    const int rc = grid_check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, ox, oy, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy;
    const GridOpts op = grid_opts2(bound, order, extrapolate);
    return launch_spline2d(op, B * nout, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_grad2d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, nx, ny, grid, Bg, nout,
                           op, B, out);
    });
}
