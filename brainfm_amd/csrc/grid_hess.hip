// interpol grid_hess / grid_pushgrad for spline orders 0 to 3, any order per axis: what makes grid_grad differentiable
// (utils/interpol/pushpull.py:303-325).  hess: nd.py:368-464, iso1.py:547-675; pushgrad, the adjoint of grad:
// nd.py:291-364, iso1.py:390-544; all-nearest calls are zero (iso0.py:326-368).
//
// The nodes, signs, weights and the launch shape are those of spline_grid.hip (axis_nodes of spline_nodes.h with its
// derivative levels 1 and 2, the prologue, checks and dispatch of grid_kernels.h): one thread per voxel, the nodes of the
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
// value is exactly 0 issues nothing.  The summation order, and so the last bit, is not reproducible; the _fixed export
// adds the same values as 64-bit fixed-point integers instead, whose sum has no order (push_accum.h).
#include "grid_kernels.h"
#include "push_accum.h"

namespace {

// O = 1, 2, 3: isotropic order O with O + 1 taps per axis (O = 1: iso1's slope); O < 0: per-axis orders from `op`, 4 taps.
// cot == nullptr: out [B][C][nout][3][3]; else cot [B][C][nout][3] and out [B][nout][3]
template <int O>
__global__ void __launch_bounds__(256) spline_hess3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op,
                                                     int B, const float* __restrict__ cot, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    constexpr bool DIAG = O != 1;                        // an all-linear call has no second derivative
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T], hx[T], hy[T], hz[T];
        axis_nodes<T, 2, O == 1>(p.g[0], ox, nx, op.bound[0], ix, wx, dx, hx);
        axis_nodes<T, 2, O == 1>(p.g[1], oy, ny, op.bound[1], iy, wy, dy, hy);
        axis_nodes<T, 2, O == 1>(p.g[2], oz, nz, op.bound[2], iz, wz, dz, hz);
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;              // the contraction, summed over the channels
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
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
            hxx *= p.mask; hyy *= p.mask; hzz *= p.mask; hxy *= p.mask; hxz *= p.mask; hyz *= p.mask;
            if (cot) {
                const float* t = cot + (((int64_t)p.b * C + c) * nout + p.v) * 3;
                const float tx = t[0], ty = t[1], tz = t[2];
                c0 = fmaf(hxx, tx, fmaf(hxy, ty, fmaf(hxz, tz, c0)));
                c1 = fmaf(hxy, tx, fmaf(hyy, ty, fmaf(hyz, tz, c1)));
                c2 = fmaf(hxz, tx, fmaf(hyz, ty, fmaf(hzz, tz, c2)));
            } else {
                float* o = out + (((int64_t)p.b * C + c) * nout + p.v) * 9;
                o[0] = hxx; o[1] = hxy; o[2] = hxz;
                o[3] = hxy; o[4] = hyy; o[5] = hyz;
                o[6] = hxz; o[7] = hyz; o[8] = hzz;
            }
        }
        if (cot) {
            float* o = out + ((int64_t)p.b * nout + p.v) * 3;
            o[0] = c0; o[1] = c1; o[2] = c2;
        }
    }
}

// inp [Bi][C][nin][3], out [B][C][nx*ny*nz] zero on entry, accumulated through ACC (push_accum.h): AccumFloat, the fp32
// atomics described above, or AccumFixed, int64 fixed-point atomics that give the same bits in every order.
// Fixed-point bound, G = 3: with m the largest |component| of the slice, val = tx (dwx wy wz) + ty (wx dwy wz) + tz (wx wy
// dwz).  The weights (times sign) lie in [-1, 1] (spline_push), and so do the derivatives at orders 1 to 3: the slope is
// +-1; the quadratic's -2|x| on |x| < 1/2 and |x| - 3/2 on 1/2 <= |x| <= 3/2 lie in [-1, 0]; the cubic's |x| (3/2 |x| - 2) on
// |x| < 1 is least at |x| = 2/3, -2/3, and its -(2 - |x|)^2 / 2 on 1 <= |x| <= 2 lies in [-1/2, 0].  Rounding is monotone, so
// every rounded product of such factors stays in [-1, 1], |pw| <= 2 m, |pd| <= m and |val| <= fl(3 m) < 3 * 2^e for m < 2^e.
template <int O, typename ACC>
__global__ void __launch_bounds__(256) spline_pushgrad3d(const float* __restrict__ inp, int Bi, int C,
                                                         const float* __restrict__ grid, int Bg, int64_t nin, int nx,
                                                         int ny, int nz, GridOpts op, int B,
                                                         typename ACC::Cell* __restrict__ out, typename ACC::Aux aux) {
    constexpr int T = grid_taps(O);
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nin;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nin, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        if (p.mask == 0.f) continue;
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T];
        axis_nodes<T, 1, O == 1>(p.g[0], ox, nx, op.bound[0], ix, wx, dx);
        axis_nodes<T, 1, O == 1>(p.g[1], oy, ny, op.bound[1], iy, wy, dy);
        axis_nodes<T, 1, O == 1>(p.g[2], oz, nz, op.bound[2], iz, wz, dz);
        for (int c = 0; c < C; ++c) {
            const int64_t sin = (int64_t)(Bi == 1 ? 0 : p.b) * C + c;
            const float* t = inp + (sin * nin + p.v) * 3;
            const float tx = t[0], ty = t[1], tz = t[2];
            typename ACC::Cell* dst = out + ((int64_t)p.b * C + c) * vol;
            const auto scale = ACC::scale(aux, sin);
            if (ACC::dead(scale)) continue;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    typename ACC::Cell* row = dst + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float pw = fmaf(tx, dx[a] * wy[bb], ty * (wx[a] * dy[bb]));      // goes with wz
                    const float pd = tz * (wx[a] * wy[bb]);                                // goes with dwz
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float val = fmaf(pw, wz[d], pd * dz[d]);
                        if (val != 0.f) ACC::add(row + iz[d], val, scale);
                    }
                }
        }
    }
}

}  // namespace

// hess / pushgrad have their own instantiation for the isotropic orders 1, 2 and 3; {0,0,0} is zero and launches nothing
template <typename F>
static int launch_hess(const int* order, int64_t n, F&& launch) {
    dispatch_order<1, 2, 3>(order, [&](auto o) { launch(o, dim3(grid_for(n)), dim3(256)); });
    return bfm_launch_status();
}

extern "C" int bfm_grid_hess3d(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg, int ox,
                               int oy, int oz, const int* bound, const int* order, int extrapolate, const float* cot,
                               float* out, bfm_stream_t stream) {
    const GridDims<3> in{{nx, ny, nz}}, og{{ox, oy, oz}};
    const int rc = grid_check_args(3, inp, grid, out, bound, order, Bi, Bg, C, in.n, og.n, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = og.count();
    if (iso_order(order) == 0) {                         // iso0.py:353-368: zeros
        const size_t count = (size_t)B * nout * (cot ? 3 : (size_t)C * 9);
        if (hipMemsetAsync(out, 0, count * sizeof(float), bfm_s(stream)) != hipSuccess) return BFM_E_LAUNCH;
        return bfm_launch_status();
    }
    const GridOpts op = grid_opts(3, bound, order, extrapolate);
    return launch_hess(order, B * nout, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL(spline_hess3d<decltype(o)::value>, gr, bl, 0, bfm_s(stream), inp, Bi, C, nx, ny, nz, grid, Bg,
                           nout, op, B, cot, out);
    });
}

extern "C" int bfm_grid_pushgrad3d(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                   int nx, int ny, int nz, const int* bound, const int* order, int extrapolate,
                                   float* out_zeroed, bfm_stream_t stream) {
    const GridDims<3> in{{ix, iy, iz}}, vol{{nx, ny, nz}};
    const int rc = grid_check_args(3, inp, grid, out_zeroed, bound, order, Bi, Bg, C, in.n, vol.n, extrapolate);
    if (rc != BFM_OK) return rc;
    if (iso_order(order) == 0) return BFM_OK;            // iso0.py:326-349: zeros, which the caller has written
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = in.count();
    const GridOpts op = grid_opts(3, bound, order, extrapolate);
    return launch_hess(order, B * nin, [&](auto o, dim3 gr, dim3 bl) {
        hipLaunchKernelGGL((spline_pushgrad3d<decltype(o)::value, AccumFloat>), gr, bl, 0, bfm_s(stream), inp, Bi, C, grid,
                           Bg, nin, nx, ny, nz, op, B, out_zeroed, AccumFloat::Aux{});
    });
}

// The same sums through int64 fixed-point accumulators in the workspace (push_fixed.hip), G = 3.  An all-nearest call
// launches no push: its accumulators stay zero and the finalize pass writes the zeros.
extern "C" int bfm_grid_pushgrad3d_fixed(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                         int nx, int ny, int nz, const int* bound, const int* order, int extrapolate,
                                         float* out, void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    const GridDims<3> in{{ix, iy, iz}}, vol{{nx, ny, nz}};
    int rc = grid_check_args(3, inp, grid, out, bound, order, Bi, Bg, C, in.n, vol.n, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = in.count();
    PushFixedPlan plan;
    rc = push_fixed_begin(&plan, inp, Bi, C, nin * 3, B, vol.count(), nin, order, 3, 3, workspace, workspace_bytes, stream);
    if (rc != BFM_OK) return rc;
    if (iso_order(order) != 0) {
        const GridOpts op = grid_opts(3, bound, order, extrapolate);
        rc = launch_hess(order, B * nin, [&](auto o, dim3 gr, dim3 bl) {
            hipLaunchKernelGGL((spline_pushgrad3d<decltype(o)::value, AccumFixed>), gr, bl, 0, bfm_s(stream), inp, Bi, C,
                               grid, Bg, nin, nx, ny, nz, op, B, plan.acc, plan.k);
        });
        if (rc != BFM_OK) return rc;
    }
    return push_fixed_end(plan, out, stream);
}
