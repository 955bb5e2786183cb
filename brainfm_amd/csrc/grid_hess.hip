// interpol grid_hess / grid_pushgrad for spline orders 0 to 3, any order per axis: what makes grid_grad differentiable
// (utils/interpol/pushpull.py:303-325).  hess: nd.py:368-464, iso1.py:547-675; pushgrad, the adjoint of grad:
// nd.py:291-364, iso1.py:390-544; all-nearest calls are zero (iso0.py:326-368).
//
// The nodes, signs, weights and the launch shape are those of spline_grid.hip: one thread per voxel, the nodes of the
// three axes in registers with the sign folded into every weight, the channel loop inside, every texel load ld_tex.
// Instantiations: the isotropic orders 1, 2 and 3 with their 2, 3 and 4 taps per axis, and the one padded to 4 x 4 x 4 taps
// for every other combination.
//
// hess entry (d, d) takes fasthess (splines.py:149-157) on axis d and the plain weights on the other two; entry (d, d2)
// takes fastgrad on both axes and the plain weight on the third; the lower triangle is the upper one.  One template
// writes either the Hessian itself, (B,C,N,3,3), or -- what the backward of grid_grad needs -- its contraction with a
// cotangent (B,C,N,3): out[b,v,j] = sum_c sum_i H[b,c,v,i,j] * cot[b,c,v,i], (B,N,3), without the 36 bytes per voxel and
// channel in between.
//
// The inbounds mask multiplies the result for every batch and channel count.  nd.hess of the reference unsqueezes the
// mask once too often (nd.py:456) and so raises, or returns a wrongly shaped result, unless B = C = 1, where it gives
// exactly this product.
//
// fastgrad at order 1 is sign(x) in the generic path (splines.py:93-97), the opposite of the true slope, and is followed as
// it stands on a linear axis of a mixed-order call (see spline_grid.hip).  An all-linear call is iso1's in the reference
// and takes the true slope: the two agree for hess (two slopes multiply, the diagonal is zero) and differ in sign for
// pushgrad, so order {1,1,1} has its own 2-tap instantiation.
//
// pushgrad: a source voxel holds a 3-vector c and adds sign * mask * (c_x dwx wy wz + c_y wx dwy wz + c_z wx wy dwz) to each
// of its nodes: one fp32 atomic per node, as many as spline_push3d issues.  out must be zero on entry; a node whose
// value is exactly 0 issues nothing.  The summation order, and so the last bit, is not reproducible.
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

// O = 1, 2, 3: isotropic order O with O + 1 taps per axis (O = 1: iso1's slope); O < 0: per-axis orders from `ord`, 4 taps.
// cot == nullptr: out [B][C][nout][3][3]; else cot [B][C][nout][3] and out [B][nout][3]
template <int O>
__global__ void __launch_bounds__(256) spline_hess3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout, Bounds bd,
                                                     Orders ord, int extrap, int B, const float* __restrict__ cot,
                                                     float* __restrict__ out) {
    constexpr int T = O < 0 ? 4 : O + 1;
    constexpr bool DIAG = O != 1;                        // an all-linear call has no second derivative
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
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T], hx[T], hy[T], hz[T];
        axis_nodes2<T, O == 1>(gx, ox, nx, bd.b[0], ix, wx, dx, hx);
        axis_nodes2<T, O == 1>(gy, oy, ny, bd.b[1], iy, wy, dy, hy);
        axis_nodes2<T, O == 1>(gz, oz, nz, bd.b[2], iz, wz, dz, hz);
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;              // the contraction, summed over the channels
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : b) * C + c) * vol;
            float hxx = 0.f, hyy = 0.f, hzz = 0.f, hxy = 0.f, hxz = 0.f, hyz = 0.f;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const float* row = src + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    float sw = 0.f, sd = 0.f, sh = 0.f;  // the row against the weights, slopes and curvatures of z
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float val = ld_tex(row + iz[d]);
                        sw = fmaf(val, wz[d], sw);
                        sd = fmaf(val, dz[d], sd);
                        if (DIAG) sh = fmaf(val, hz[d], sh);
                    }
                    if (DIAG) {
                        hxx = fmaf(hx[a] * wy[bb], sw, hxx);
                        hyy = fmaf(wx[a] * hy[bb], sw, hyy);
                        hzz = fmaf(wx[a] * wy[bb], sh, hzz);
                    }
                    hxy = fmaf(dx[a] * dy[bb], sw, hxy);
                    hxz = fmaf(dx[a] * wy[bb], sd, hxz);
                    hyz = fmaf(wx[a] * dy[bb], sd, hyz);
                }
            hxx *= mask; hyy *= mask; hzz *= mask; hxy *= mask; hxz *= mask; hyz *= mask;
            if (cot) {
                const float* t = cot + (((int64_t)b * C + c) * nout + v) * 3;
                const float tx = t[0], ty = t[1], tz = t[2];
                c0 = fmaf(hxx, tx, fmaf(hxy, ty, fmaf(hxz, tz, c0)));
                c1 = fmaf(hxy, tx, fmaf(hyy, ty, fmaf(hyz, tz, c1)));
                c2 = fmaf(hxz, tx, fmaf(hyz, ty, fmaf(hzz, tz, c2)));
            } else {
                float* o = out + (((int64_t)b * C + c) * nout + v) * 9;
                o[0] = hxx; o[1] = hxy; o[2] = hxz;
                o[3] = hxy; o[4] = hyy; o[5] = hyz;
                o[6] = hxz; o[7] = hyz; o[8] = hzz;
            }
        }
        if (cot) {
            float* o = out + ((int64_t)b * nout + v) * 3;
            o[0] = c0; o[1] = c1; o[2] = c2;
        }
    }
}

// inp [Bi][C][nin][3], out [B][C][nx*ny*nz] zero on entry
template <int O>
__global__ void __launch_bounds__(256) spline_pushgrad3d(const float* __restrict__ inp, int Bi, int C,
                                                         const float* __restrict__ grid, int Bg, int64_t nin, int nx,
                                                         int ny, int nz, Bounds bd, Orders ord, int extrap, int B,
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
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T], unused[T];
        axis_nodes2<T, O == 1>(gx, ox, nx, bd.b[0], ix, wx, dx, unused);
        axis_nodes2<T, O == 1>(gy, oy, ny, bd.b[1], iy, wy, dy, unused);
        axis_nodes2<T, O == 1>(gz, oz, nz, bd.b[2], iz, wz, dz, unused);
        for (int c = 0; c < C; ++c) {
            const float* t = inp + (((int64_t)(Bi == 1 ? 0 : b) * C + c) * nin + v) * 3;
            const float tx = t[0], ty = t[1], tz = t[2];
            float* dst = out + ((int64_t)b * C + c) * vol;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    float* row = dst + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float pw = fmaf(tx, dx[a] * wy[bb], ty * (wx[a] * dy[bb]));      // goes with wz
                    const float pd = tz * (wx[a] * wy[bb]);                                // goes with dwz
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float val = fmaf(pw, wz[d], pd * dz[d]);
                        if (val != 0.f) atomicAdd(row + iz[d], val);
                    }
                }
        }
    }
}

// the argument checks of spline_grid.hip's check_args
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

// 0 to 3 for an isotropic order, -1 for the padded instantiation
int iso_order(const int* o) { return (o[0] == o[1] && o[1] == o[2]) ? o[0] : -1; }

}  // namespace

#define BFM_HESS_LAUNCH(KERNEL, N, ...)                                                                                \
    do {                                                                                                               \
        const int iso = iso_order(order);                                                                              \
        const dim3 gr(grid_for(N)), bl(256);                                                                           \
        if (iso == 1) hipLaunchKernelGGL(KERNEL<1>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                            \
        else if (iso == 2) hipLaunchKernelGGL(KERNEL<2>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                       \
        else if (iso == 3) hipLaunchKernelGGL(KERNEL<3>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                       \
        else hipLaunchKernelGGL(KERNEL<-1>, gr, bl, 0, bfm_s(stream), __VA_ARGS__);                                    \
    } while (0)

extern "C" int bfm_grid_hess3d(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                               int oy, int oz, const int* bound, const int* order, int extrapolate, const float* cot,
                               float* out, bfm_stream_t stream) {
    const int rc = check_args(inp, grid, out, bound, order, Bi, Bg, C, nx, ny, nz, ox, oy, oz, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = (int64_t)ox * oy * oz;
    if (iso_order(order) == 0) {                         // iso0.py:353-368: zeros
        const size_t count = (size_t)B * nout * (cot ? 3 : (size_t)C * 9);
        if (hipMemsetAsync(out, 0, count * sizeof(float), bfm_s(stream)) != hipSuccess) return BFM_E_LAUNCH;
        return bfm_launch_status();
    }
    const Bounds bd{{bound[0], bound[1], bound[2]}};
    const Orders od{{order[0], order[1], order[2]}};
    BFM_HESS_LAUNCH(spline_hess3d, B * nout, inp, Bi, C, nx, ny, nz, grid, Bg, nout, bd, od, extrapolate, B, cot, out);
    return bfm_launch_status();
}

extern "C" int bfm_grid_pushgrad3d(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                   int nx, int ny, int nz, const int* bound, const int* order, int extrapolate,
                                   float* out_zeroed, bfm_stream_t stream) {
    const int rc = check_args(inp, grid, out_zeroed, bound, order, Bi, Bg, C, ix, iy, iz, nx, ny, nz, extrapolate);
    if (rc != BFM_OK) return rc;
    if (iso_order(order) == 0) return BFM_OK;            // iso0.py:326-349: zeros, which the caller has written
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = (int64_t)ix * iy * iz;
    const Bounds bd{{bound[0], bound[1], bound[2]}};
    const Orders od{{order[0], order[1], order[2]}};
    BFM_HESS_LAUNCH(spline_pushgrad3d, B * nin, inp, Bi, C, grid, Bg, nin, nx, ny, nz, bd, od, extrapolate, B, out_zeroed);
    return bfm_launch_status();
}
