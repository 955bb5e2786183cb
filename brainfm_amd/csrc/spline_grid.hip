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
// runs the instantiation padded to 4 x 4 x 4 taps, where an unused tap has weight 0 and the index of tap 0.
//
// fastgrad at order 1 is sign(x) (splines.py:93-97), the opposite sign of iso1.grad3d's -1 / +1: the reference's generic
// path is followed as it stands.  It shows only on a linear axis of a mixed-order call; all-linear calls go to the
// linear kernels of synth_interp.hip.
//
// The sums are ((wx * wy) * wz) * value accumulated tap by tap (x slowest), where the reference multiplies the value by
// the three weights in turn: the same terms, rounded differently in the last bit.
#include "bfm_common.h"
#include "gather3d.h"
#include "interp_bounds.h"
#include "spline_nodes.h"

namespace {

inline int grid_for(int64_t n, int tpb = 256, int cap = 8192) {
    int64_t b = bfm_cdiv64(n, tpb);
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

#define GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

struct Orders { int o[3]; };
struct Bounds { int b[3]; };

// O = 0, 2, 3: isotropic order O with O + 1 taps per axis; O < 0: per-axis orders from `ord`, 4 taps per axis
template <int O>
__global__ void __launch_bounds__(256) spline_pull3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout, Bounds bd,
                                                     Orders ord, int extrap, int B, float* __restrict__ out) {
    constexpr int T = O < 0 ? 4 : O + 1;
    const int ox = O < 0 ? ord.o[0] : O, oy = O < 0 ? ord.o[1] : O, oz = O < 0 ? ord.o[2] : O;
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / nout);
        const int64_t v = i - (int64_t)b * nout;
        const float* g = grid + ((int64_t)(Bg == 1 ? 0 : b) * nout + v) * 3;
        const float gx = ld_tex(g), gy = ld_tex(g + 1), gz = ld_tex(g + 2);
        const float mask = inbounds(gx, gy, gz, nx, ny, nz, extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], unused[T];
        axis_nodes<T, false>(gx, ox, nx, bd.b[0], ix, wx, unused);
        axis_nodes<T, false>(gy, oy, ny, bd.b[1], iy, wy, unused);
        axis_nodes<T, false>(gz, oz, nz, bd.b[2], iz, wz, unused);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : b) * C + c) * vol;
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
            out[((int64_t)b * C + c) * nout + v] = acc * mask;
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
                                                     int nz, Bounds bd, Orders ord, int extrap, int B,
                                                     float* __restrict__ out) {
    constexpr int T = O < 0 ? 4 : O + 1;
    const int ox = O < 0 ? ord.o[0] : O, oy = O < 0 ? ord.o[1] : O, oz = O < 0 ? ord.o[2] : O;
    const int64_t n = (int64_t)B * nin;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / nin);
        const int64_t v = i - (int64_t)b * nin;
        const float* g = grid + ((int64_t)(Bg == 1 ? 0 : b) * nin + v) * 3;
        const float gx = ld_tex(g), gy = ld_tex(g + 1), gz = ld_tex(g + 2);
        const float mask = inbounds(gx, gy, gz, nx, ny, nz, extrap);
        if (mask == 0.f) continue;
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], unused[T];
        axis_nodes<T, false>(gx, ox, nx, bd.b[0], ix, wx, unused);
        axis_nodes<T, false>(gy, oy, ny, bd.b[1], iy, wy, unused);
        axis_nodes<T, false>(gz, oz, nz, bd.b[2], iz, wz, unused);
        for (int c = 0; c < C; ++c) {
            const float val = inp[((int64_t)(Bi == 1 ? 0 : b) * C + c) * nin + v];
            float* dst = out + ((int64_t)b * C + c) * vol;
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
                                                     const float* __restrict__ grid, int Bg, int64_t nout, Bounds bd,
                                                     Orders ord, int extrap, int B, float* __restrict__ out) {
    constexpr int T = O < 0 ? 4 : O + 1;
    const int ox = O < 0 ? ord.o[0] : O, oy = O < 0 ? ord.o[1] : O, oz = O < 0 ? ord.o[2] : O;
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / nout);
        const int64_t v = i - (int64_t)b * nout;
        const float* g = grid + ((int64_t)(Bg == 1 ? 0 : b) * nout + v) * 3;
        const float gx = ld_tex(g), gy = ld_tex(g + 1), gz = ld_tex(g + 2);
        const float mask = inbounds(gx, gy, gz, nx, ny, nz, extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T];
        axis_nodes<T, true>(gx, ox, nx, bd.b[0], ix, wx, dx);
        axis_nodes<T, true>(gy, oy, ny, bd.b[1], iy, wy, dy);
        axis_nodes<T, true>(gz, oz, nz, bd.b[2], iz, wz, dz);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : b) * C + c) * vol;
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
            float* o = out + (((int64_t)b * C + c) * nout + v) * 3;
            o[0] = ax * mask; o[1] = ay * mask; o[2] = az * mask;
        }
    }
}

// the argument checks of the _linear exports (synth_interp.hip) plus the orders
int check_args(const void* inp, const void* grid, const void* out, const int* bound, const int* order, int Bi, int Bg,
               int C, int a0, int a1, int a2, int b0, int b1, int b2, int extrapolate) {
    if (!inp || !grid || !out || !bound || !order || Bi <= 0 || Bg <= 0 || C <= 0 || a0 <= 0 || a1 <= 0 || a2 <= 0 ||
        b0 <= 0 || b1 <= 0 || b2 <= 0)
        return BFM_E_ARG;
    if (Bi != Bg && Bi != 1 && Bg != 1) return BFM_E_SHAPE;
    for (int a = 0; a < 3; ++a) if (bound[a] < 0 || bound[a] > 6) return BFM_E_ARG;
    for (int a = 0; a < 3; ++a) if (order[a] < 0 || order[a] > 3) return BFM_E_ARG;
    if (extrapolate < 0 || extrapolate > 2) return BFM_E_ARG;
    return BFM_OK;
}

// 0, 2, 3 for an isotropic order with its own instantiation, -1 for the padded one
int iso_order(const int* o) { return (o[0] == o[1] && o[1] == o[2] && o[0] != 1) ? o[0] : -1; }

}  // namespace

#define BFM_SPLINE_LAUNCH(KERNEL, N, ...)                                                                              \
    do {                                                                                                               \
        const int iso = iso_order(order);                                                                              \
        const dim3 gr(grid_for(N)), bl(256);                                                                           \
        if (iso == 0) hipLaunchKernelGGL(KERNEL<0>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                            \
        else if (iso == 2) hipLaunchKernelGGL(KERNEL<2>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                       \
        else if (iso == 3) hipLaunchKernelGGL(KERNEL<3>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                       \
        else hipLaunchKernelGGL(KERNEL<-1>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                                    \
    } while (0)

extern "C" int bfm_grid_pull3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, const int* order,
                                      int extrapolate, float* out, bfm_stream_t stream) {
    const int rc = check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, nz, ox, oy, oz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy * oz;
    const Bounds bd{{bound[0], bound[1], bound[2]}};
    const Orders od{{order[0], order[1], order[2]}};
    BFM_SPLINE_LAUNCH(spline_pull3d, B * nout, inp, Bi, C, nx, ny, nz, grid, Bg, nout, bd, od, extrapolate, B, out);
    return bfm_launch_status();
}

extern "C" int bfm_grid_push3d_spline(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                      int nx, int ny, int nz, const int* bound, const int* order, int extrapolate,
                                      float* out_zeroed, bfm_stream_t stream) {
    const int rc = check_args(inp, grid, out_zeroed, bound, order, Bi, Bg, C, ix, iy, iz, nx, ny, nz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = (int64_t)ix * iy * iz;
    const Bounds bd{{bound[0], bound[1], bound[2]}};
    const Orders od{{order[0], order[1], order[2]}};
    BFM_SPLINE_LAUNCH(spline_push3d, B * nin, inp, Bi, C, grid, Bg, nin, nx, ny, nz, bd, od, extrapolate, B, out_zeroed);
    return bfm_launch_status();
}

extern "C" int bfm_grid_grad3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, const int* order,
                                      int extrapolate, float* out, bfm_stream_t stream) {
    const int rc = check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, nz, ox, oy, oz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy * oz;
    const Bounds bd{{bound[0], bound[1], bound[2]}};
    const Orders od{{order[0], order[1], order[2]}};
    BFM_SPLINE_LAUNCH(spline_grad3d, B * nout, inp, Bi, C, nx, ny, nz, grid, Bg, nout, bd, od, extrapolate, B, out);
    return bfm_launch_status();
}
