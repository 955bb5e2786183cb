// interpol grid_pull / grid_push / grid_grad for spline orders 0 to 3, any order per axis: the generic path of the
// vendored torch-interpol (utils/interpol/nd.py:30-290, splines.py:30-43 and :90-103, bounds.py:24-89).
//
// Per axis of order o: grid0 = floor(g - (o-1)/2); node k in 0..o sits at grid0 + k, is read at bound_index(grid0 + k),
// takes bound_sign(grid0 + k) and the weight fastweight(g - grid0 - k); grad replaces the weight of its own axis by
// fastgrad.  The inbounds mask has the thresholds of the linear kernels (extrapolate 0 no / 1 yes / 2 hist).
//
// One thread per output voxel (pull, grad) or per source voxel (push).  Nodes, signs and weights are computed once per
// voxel and stay in registers, the sign folded into the weight (a factor of -1, 0 or 1 is exact); the channel loop is
// inside.  Every texel load is ld_tex (gather3d.h).  The isotropic orders 0, 2 and 3 are instantiated with their tap
// counts (1, 3, 4 per axis), so every array is indexed by constants and nothing goes to scratch; any other combination
// runs the instantiation padded to 4 x 4 x 4 taps, where an unused tap has weight 0 and the index of tap 0.  The nodes are
// axis_nodes of spline_nodes.h; the voxel prologue, the options struct, the argument checks and the dispatch from the
// orders to an instantiation are grid_kernels.h, shared with grid_hess.hip and label_pull.hip.
//
// fastgrad at order 1 is sign(x) (splines.py:93-97), the opposite sign of iso1.grad3d's -1 / +1: the reference's generic
// path is followed as it stands.  It shows only on a linear axis of a mixed-order call; all-linear calls go to the
// linear kernels of synth_interp.hip.
//
// The sums are ((wx * wy) * wz) * value accumulated tap by tap (x slowest), where the reference multiplies the value by
// the three weights in turn: the same terms, rounded differently in the last bit.
#include "grid_kernels.h"

namespace {

// O = 0, 2, 3: isotropic order O with O + 1 taps per axis; O < 0: per-axis orders from `op`, 4 taps per axis
template <int O>
__global__ void __launch_bounds__(256) spline_pull3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout,
                                                     GridOpts op, int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridVoxel p = grid_voxel(i, nout, grid, Bg, nx, ny, nz, op.extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T];
        axis_nodes<T>(p.gx, ox, nx, op.bound[0], ix, wx);
        axis_nodes<T>(p.gy, oy, ny, op.bound[1], iy, wy);
        axis_nodes<T>(p.gz, oz, nz, op.bound[2], iz, wz);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const float* row = src + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float wxy = wx[a] * wy[bb];
#pragma unroll
                    for (int d = 0; d < T; ++d) acc = fmaf(ld_tex(row + iz[d]), wxy * wz[d], acc);
                }
            out[((int64_t)p.b * C + c) * nout + p.v] = acc * p.mask;
        }
    }
}

// nd.push: the adjoint of pull -- every source voxel scatters its value to its nodes.  out [B][C][nx*ny*nz] must be zero on
// entry.  fp32 atomics (one global_atomic_add_f32 each): the summation order, and so the last bit, is not reproducible.  A
// tap whose weight times sign is exactly 0 (a node the `zero` bound drops, a padded tap, a masked voxel) issues nothing.
// The taps are the outer loops and the lanes run along the fastest axis of the source, so for a smooth grid one atomic
// wave-instruction covers neighbouring addresses of a few rows.
template <int O>
__global__ void __launch_bounds__(256) spline_push3d(const float* __restrict__ inp, int Bi, int C,
                                                     const float* __restrict__ grid, int Bg, int64_t nin, int nx, int ny,
                                                     int nz, GridOpts op, int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nin;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridVoxel p = grid_voxel(i, nin, grid, Bg, nx, ny, nz, op.extrap);
        if (p.mask == 0.f) continue;
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T];
        axis_nodes<T>(p.gx, ox, nx, op.bound[0], ix, wx);
        axis_nodes<T>(p.gy, oy, ny, op.bound[1], iy, wy);
        axis_nodes<T>(p.gz, oz, nz, op.bound[2], iz, wz);
        for (int c = 0; c < C; ++c) {
            const float val = inp[((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * nin + p.v];
            float* dst = out + ((int64_t)p.b * C + c) * vol;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    float* row = dst + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float wxy = wx[a] * wy[bb];
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float w = wxy * wz[d];
                        if (w != 0.f) atomicAdd(row + iz[d], val * w);
                    }
                }
        }
    }
}

// nd.grad: out [B][C][nout][3]; component d takes fastgrad on axis d and the plain weights on the other two
template <int O>
__global__ void __launch_bounds__(256) spline_grad3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout,
                                                     GridOpts op, int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridVoxel p = grid_voxel(i, nout, grid, Bg, nx, ny, nz, op.extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T];
        axis_nodes<T, 1>(p.gx, ox, nx, op.bound[0], ix, wx, dx);
        axis_nodes<T, 1>(p.gy, oy, ny, op.bound[1], iy, wy, dy);
        axis_nodes<T, 1>(p.gz, oz, nz, op.bound[2], iz, wz, dz);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const float* row = src + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float gxy = dx[a] * wy[bb], xgy = wx[a] * dy[bb], wxy = wx[a] * wy[bb];
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float val = ld_tex(row + iz[d]);
                        ax = fmaf(val, gxy * wz[d], ax);
                        ay = fmaf(val, xgy * wz[d], ay);
                        az = fmaf(val, wxy * dz[d], az);
                    }
                }
            float* o = out + (((int64_t)p.b * C + c) * nout + p.v) * 3;
            o[0] = ax * p.mask; o[1] = ay * p.mask; o[2] = az * p.mask;
        }
    }
}

}  // namespace

// pull / push / grad have their own instantiation for the isotropic orders 0, 2 and 3; {1,1,1} runs the padded one here
// (the reference's generic path), and interpol.py sends all-linear calls to the _linear exports instead
template <typename F>
static int launch_spline(const int* order, int64_t n, F&& launch) {
    dispatch_order<0, 2, 3>(order, [&](auto o) { launch(o, dim3(grid_for(n)), dim3(256)); });
    return bfm_launch_status();
}

extern "C" int bfm_grid_pull3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, const int* order,
                                      int extrapolate, float* out, bfm_stream_t stream) {
    const int rc = grid_check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, nz, ox, oy, oz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy * oz;
    const GridOpts op = grid_opts(bound, order, extrapolate);
    return launch_spline(order, B * nout, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_pull3d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, nx, ny, nz, grid, Bg,
                           nout, op, B, out);
    });
}

extern "C" int bfm_grid_push3d_spline(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                      int nx, int ny, int nz, const int* bound, const int* order, int extrapolate,
                                      float* out_zeroed, bfm_stream_t stream) {
    const int rc = grid_check_args(inp, grid, out_zeroed, bound, order, Bi, Bg, C, ix, iy, iz, nx, ny, nz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = (int64_t)ix * iy * iz;
    const GridOpts op = grid_opts(bound, order, extrapolate);
    return launch_spline(order, B * nin, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_push3d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, grid, Bg, nin, nx, ny,
                           nz, op, B, out_zeroed);
    });
}

extern "C" int bfm_grid_grad3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, const int* order,
                                      int extrapolate, float* out, bfm_stream_t stream) {
    const int rc = grid_check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, nz, ox, oy, oz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy * oz;
    const GridOpts op = grid_opts(bound, order, extrapolate);
    return launch_spline(order, B * nout, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_grad3d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, nx, ny, nz, grid, Bg,
                           nout, op, B, out);
    });
}
