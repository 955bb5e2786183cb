// interpol grid_pull / grid_push / grid_grad on 2-D and 3-D grids for spline orders 0 to 3, any order per axis: the generic
// path of the vendored torch-interpol (utils/interpol/nd.py:30-290, splines.py:30-43 and :90-103, bounds.py:24-89), which
// on a 2-D grid also computes what iso0.pull2d / push2d and iso1.pull2d / push2d / grad2d do, and the three all-linear
// 3-D kernels of iso1.py (iso1.py:28-387) at the end of the file.
//
// Layouts: image [B][C][*n], grid [Bg][*out][D], gradient [B][C][nout][D]; D = 2 or 3 is a template parameter and the
// extents *n reach a kernel as one GridDims<D>.
//
// Per axis of order o: grid0 = floor(g - (o-1)/2); node k in 0..o sits at grid0 + k, is read at bound_index(grid0 + k),
// takes bound_sign(grid0 + k) and the weight fastweight(g - grid0 - k); grad replaces the weight of its own axis by
// fastgrad.  The inbounds mask has the thresholds of extrapolate 0 no / 1 yes / 2 hist.
//
// One thread per grid point (the output of pull / grad, the source of push).  Nodes, signs and weights are computed once
// per point and stay in registers, the sign folded into the weight (a factor of -1, 0 or 1 is exact); the channel loop is
// inside.  Every texel and coordinate load is ld_tex (gather3d.h).  An isotropic order O that has its own instantiation
// runs O + 1 taps per axis, so every array is indexed by constants and nothing goes to scratch; any other combination
// runs the instantiation padded to 4 taps per axis, where an unused tap has weight 0 and the index of tap 0.  3-D
// instantiates the orders 0, 2 and 3 (all-linear calls go to the linear kernels below) and runs every other combination,
// an all-linear call that reaches a _spline export included, on the three padded kernels with spelled-out axes further
// down; 2-D instantiates the orders 0 to 3 and the padded one.  The nodes are axis_nodes of spline_nodes.h; the point prologue,
// the options struct, the argument checks and the dispatch are grid_kernels.h, shared with grid_hess.hip and
// label_pull.hip.
//
// fastgrad at order 1 is sign(x) (splines.py:93-97), the opposite sign of iso1's slope (-1 at the lower node, +1 at the
// upper): the reference's generic path is followed as it stands.  It shows only on a linear axis of a mixed-order call.
// An all-linear call takes iso1's slope, as in the reference: in 3-D on the linear kernels, in 2-D in the order-1
// instantiation of spline_grad.
//
// The sums are ((w0 * w1) * w2) * value accumulated tap by tap (axis 0 slowest), the mask last, where the reference
// multiplies the value by the weights in turn: the same terms, rounded differently in the last bit.  A 2-D call has the
// terms and the order of the 3-D one on the image [nx][ny][1] with a third coordinate 0 and order 0 on the third axis,
// whose extra factor is an exact 1 and whose padded taps add exact zeros.
#include "grid_kernels.h"
#include "push_accum.h"

namespace {

// The taps of a footprint, axis 0 slowest: f(offset, wt) with offset = (..(idx[0][k0] * n[1] + idx[1][k1]) * n[2] + ..) and
// the weights folded left to right.  NW == 1: wt[0] = (w[0][k0] * w[1][k1]) * ..; NW == D (grad): wt[d] is that product with
// dw on axis d in the place of w.
template <int D, int T, int NW, int A, typename F>
__device__ __forceinline__ void tap_walk(const GridDims<D>& dims, const int (&idx)[D][T], const float (&w)[D][T],
                                         const float (*dw)[T], int64_t off, const float (&wt)[NW], F&& f) {
    if constexpr (A == D) {
        f(off, wt);
    } else {
#pragma unroll
        for (int k = 0; k < T; ++k) {
            float next[NW];
#pragma unroll
            for (int d = 0; d < NW; ++d) {
                const float factor = (NW > 1 && d == A) ? dw[A][k] : w[A][k];
                next[d] = A == 0 ? factor : wt[d] * factor;
            }
            tap_walk<D, T, NW, A + 1>(dims, idx, w, dw, off * dims.n[A] + idx[A][k], next, f);
        }
    }
}

template <int D, int T, int NW, typename F>
__device__ __forceinline__ void for_each_tap(const GridDims<D>& dims, const int (&idx)[D][T], const float (&w)[D][T],
                                             const float (*dw)[T], F&& f) {
    const float none[NW] = {};
    tap_walk<D, T, NW, 0>(dims, idx, w, dw, 0, none, f);
}

// The nodes of every axis of a point, DER = 1 with their derivatives: one axis_nodes call per axis, axis by axis at compile
// time like tap_walk.  (A loop over the axes, though fully unrolled, left the padded instantiations with another branch
// structure than the three calls they had, and measurably slower: profiles/grid_nd_refactor.txt.)
template <int D, int T, int O, int DER = 0, bool ISO1 = false, int A = 0>
__device__ __forceinline__ void point_nodes(const GridPoint<D>& p, const GridDims<D>& dims, const GridOpts& op,
                                            int (&idx)[D][T], float (&w)[D][T], float (*dw)[T] = nullptr) {
    if constexpr (A < D) {
        axis_nodes<T, DER, ISO1>(p.g[A], axis_order<O>(op, A), dims.n[A], op.bound[A], idx[A], w[A], DER ? dw[A] : nullptr);
        point_nodes<D, T, O, DER, ISO1, A + 1>(p, dims, op, idx, w, dw);
    }
}

// O >= 0: isotropic order O with O + 1 taps per axis; O < 0: per-axis orders from `op`, 4 taps per axis
template <int D, int O>
__global__ void __launch_bounds__(256) spline_pull(const float* __restrict__ inp, int Bi, int C, GridDims<D> dims,
                                                   const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op,
                                                   int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = dims.count();
    GRID_STRIDE(i, n) {
        const GridPoint<D> p = grid_point<D>(i, nout, grid, Bg, dims, op.extrap);
        int idx[D][T];
        float w[D][T];
        point_nodes<D, T, O>(p, dims, op, idx, w);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            float acc = 0.f;
            for_each_tap<D, T, 1>(dims, idx, w, nullptr,
                              [&](int64_t off, const float (&wt)[1]) { acc = fmaf(ld_tex(src + off), wt[0], acc); });
            out[((int64_t)p.b * C + c) * nout + p.v] = acc * p.mask;
        }
    }
}

// nd.push: the adjoint of pull -- every source point scatters its value to its nodes.  out [B][C][*n] must be zero on
// entry.  ACC = AccumFloat: fp32 atomics (one global_atomic_add_f32 each), the summation order, and so the last bit, is
// not reproducible; ACC = AccumFixed: int64 fixed-point atomics, the same bits in every order (push_accum.h).  A
// tap whose weight times sign is exactly 0 (a node the `zero` bound drops, a padded tap) issues nothing, and neither does
// a masked point.  The taps are the outer loops and the lanes run along the fastest axis of the source, so for a smooth
// grid one atomic wave-instruction covers neighbouring addresses of a few rows.
// Fixed-point bound, G = 1: a contribution is val * wt, wt a product of at most D factors weight * sign.  The weights of
// spline_weight lie in [0, 1] at every order (1, 1 - |x| on |x| <= 1, at most 3/4 and 2/3 for the quadratic and the cubic),
// the sign is -1, 0 or 1, and a rounded product of factors in [-1, 1] stays in [-1, 1]: |val * wt| <= |val| <= m.
template <int D, int O, typename ACC>
__global__ void __launch_bounds__(256) spline_push(const float* __restrict__ inp, int Bi, int C,
                                                   const float* __restrict__ grid, int Bg, int64_t nin, GridDims<D> dims,
                                                   GridOpts op, int B, typename ACC::Cell* __restrict__ out,
                                                   typename ACC::Aux aux) {
    constexpr int T = grid_taps(O);
    const int64_t n = (int64_t)B * nin;
    const int64_t vol = dims.count();
    GRID_STRIDE(i, n) {
        const GridPoint<D> p = grid_point<D>(i, nin, grid, Bg, dims, op.extrap);
        if (p.mask == 0.f) continue;
        int idx[D][T];
        float w[D][T];
        point_nodes<D, T, O>(p, dims, op, idx, w);
        for (int c = 0; c < C; ++c) {
            const int64_t sin = (int64_t)(Bi == 1 ? 0 : p.b) * C + c;
            const float val = inp[sin * nin + p.v];
            typename ACC::Cell* dst = out + ((int64_t)p.b * C + c) * vol;
            const auto scale = ACC::scale(aux, sin);
            if (ACC::dead(scale)) continue;
            for_each_tap<D, T, 1>(dims, idx, w, nullptr, [&](int64_t off, const float (&wt)[1]) {
                if (wt[0] != 0.f) ACC::add(dst + off, val * wt[0], scale);
            });
        }
    }
}

// nd.grad: out [B][C][nout][D]; component d takes fastgrad on axis d and the plain weights on the other axes.  2-D order 1:
// iso1's slope.
template <int D, int O>
__global__ void __launch_bounds__(256) spline_grad(const float* __restrict__ inp, int Bi, int C, GridDims<D> dims,
                                                   const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op,
                                                   int B, float* __restrict__ out) {
    constexpr int T = grid_taps(O);
    constexpr bool ISO1 = D == 2 && O == 1;
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = dims.count();
    GRID_STRIDE(i, n) {
        const GridPoint<D> p = grid_point<D>(i, nout, grid, Bg, dims, op.extrap);
        int idx[D][T];
        float w[D][T], dw[D][T];
        point_nodes<D, T, O, 1, ISO1>(p, dims, op, idx, w, dw);
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            float acc[D] = {};
            for_each_tap<D, T, D>(dims, idx, w, dw, [&](int64_t off, const float (&wt)[D]) {
                const float val = ld_tex(src + off);
#pragma unroll
                for (int d = 0; d < D; ++d) acc[d] = fmaf(val, wt[d], acc[d]);
            });
            float* o = out + (((int64_t)p.b * C + c) * nout + p.v) * D;
#pragma unroll
            for (int d = 0; d < D; ++d) o[d] = acc[d] * p.mask;
        }
    }
}

// ------------------------------------------------------------------------------------------ mixed orders, 3-D: padded
// What spline_pull / push / grad<3, -1> compute, with the three axes spelled out and the extents as three scalar kernel
// arguments: in this form the padded 3-D instantiation compiles to the instructions it had before the kernels became
// dimension-generic, line for line.  The generic form gives the same bits at the same registers in another instruction
// order, and the padded 3-D calls measured 0.3 to 0.8 % slower in it (profiles/grid_nd_refactor.txt).  So a 3-D call of
// mixed orders runs these three, and the generic kernels serve every other instantiation.
__global__ void __launch_bounds__(256) padded_pull3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout,
                                                     GridOpts op, int B, float* __restrict__ out) {
    constexpr int T = 4;
    const int ox = op.order[0], oy = op.order[1], oz = op.order[2];
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T];
        axis_nodes<T>(p.g[0], ox, nx, op.bound[0], ix, wx);
        axis_nodes<T>(p.g[1], oy, ny, op.bound[1], iy, wy);
        axis_nodes<T>(p.g[2], oz, nz, op.bound[2], iz, wz);
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

template <typename ACC>
__global__ void __launch_bounds__(256) padded_push3d(const float* __restrict__ inp, int Bi, int C,
                                                     const float* __restrict__ grid, int Bg, int64_t nin, int nx, int ny,
                                                     int nz, GridOpts op, int B,
                                                     typename ACC::Cell* __restrict__ out, typename ACC::Aux aux) {
    constexpr int T = 4;
    const int ox = op.order[0], oy = op.order[1], oz = op.order[2];
    const int64_t n = (int64_t)B * nin;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nin, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        if (p.mask == 0.f) continue;
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T];
        axis_nodes<T>(p.g[0], ox, nx, op.bound[0], ix, wx);
        axis_nodes<T>(p.g[1], oy, ny, op.bound[1], iy, wy);
        axis_nodes<T>(p.g[2], oz, nz, op.bound[2], iz, wz);
        for (int c = 0; c < C; ++c) {
            const int64_t sin = (int64_t)(Bi == 1 ? 0 : p.b) * C + c;
            const float val = inp[sin * nin + p.v];
            typename ACC::Cell* dst = out + ((int64_t)p.b * C + c) * vol;
            const auto scale = ACC::scale(aux, sin);
            if (ACC::dead(scale)) continue;
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    typename ACC::Cell* cells = dst + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float wxy = wx[a] * wy[bb];
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float w = wxy * wz[d];
                        if (w != 0.f) ACC::add(cells + iz[d], val * w, scale);
                    }
                }
        }
    }
}

__global__ void __launch_bounds__(256) padded_grad3d(const float* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                     const float* __restrict__ grid, int Bg, int64_t nout,
                                                     GridOpts op, int B, float* __restrict__ out) {
    constexpr int T = 4;
    const int ox = op.order[0], oy = op.order[1], oz = op.order[2];
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        int ix[T], iy[T], iz[T];
        float wx[T], wy[T], wz[T], dx[T], dy[T], dz[T];
        axis_nodes<T, 1>(p.g[0], ox, nx, op.bound[0], ix, wx, dx);
        axis_nodes<T, 1>(p.g[1], oy, ny, op.bound[1], iy, wy, dy);
        axis_nodes<T, 1>(p.g[2], oz, nz, op.bound[2], iz, wz, dz);
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

// ---------------------------------------------------------------------------------------------- all-linear, 3-D: iso1.py
// The arithmetic of iso1.pull3d / push3d / grad3d, not the generic path's at order 1: node 1 weighs g - floor(g) (not
// 1 - |d|), the value takes the product of the three signs before the weight, pull adds value * weight without fmaf and
// assigns its first term, push issues all 8 atomics with the mask multiplied in.  Everything around that arithmetic is
// the family's.  Corner order: 000, 001, 010, 011, 100, 101, 110, 111 (x slowest).
#define LINEAR_CORNERS(a, bb, d) \
    _Pragma("unroll") for (int a = 0; a < 2; ++a) \
    _Pragma("unroll") for (int bb = 0; bb < 2; ++bb) \
    _Pragma("unroll") for (int d = 0; d < 2; ++d)

// the two nodes of every axis: index, sign and weight
struct LinearNodes { int idx[3][2], sg[3][2]; float w[3][2]; };

__device__ __forceinline__ LinearNodes linear_nodes(const GridPoint<3>& p, const GridDims<3>& dims, const GridOpts& op) {
    LinearNodes q;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = floorf(p.g[a]), t = p.g[a] - f;
        const int i0 = (int)f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            q.idx[a][k] = bound_index(i0 + k, dims.n[a], op.bound[a]);
            q.sg[a][k] = bound_sign(i0 + k, dims.n[a], op.bound[a]);
            q.w[a][k] = k == 0 ? 1.f - t : t;
        }
    }
    return q;
}

__device__ __forceinline__ int64_t linear_offset(const LinearNodes& q, const GridDims<3>& dims, int a, int bb, int d) {
    return ((int64_t)q.idx[0][a] * dims.n[1] + q.idx[1][bb]) * dims.n[2] + q.idx[2][d];
}

// iso1.pull3d (iso1.py:28-133)
__global__ void linear_pull3d(const float* __restrict__ inp, int Bi, int C, GridDims<3> dims,
                              const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op, int B,
                              float* __restrict__ out) {
    const int64_t n = (int64_t)B * nout;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, dims, op.extrap);
        const LinearNodes q = linear_nodes(p, dims, op);
        const int64_t vol = dims.count();
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            float acc = 0.f;
            bool first = true;
            LINEAR_CORNERS(a, bb, d) {
                float val = ld_tex(src + linear_offset(q, dims, a, bb, d));
                val = val * (float)(q.sg[0][a] * q.sg[1][bb] * q.sg[2][d]);
                val = val * ((q.w[0][a] * q.w[1][bb]) * q.w[2][d]);
                acc = first ? val : acc + val;
                first = false;
            }
            out[((int64_t)p.b * C + c) * nout + p.v] = acc * p.mask;
        }
    }
}

// iso1.push3d (iso1.py:136-265): the adjoint of pull3d -- every source voxel scatters its value to the 8 corners around
// its grid coordinate.  out [B][C][nx*ny*nz] must be zero on entry.  ACC = AccumFloat: fp32 atomics, the summation order
// (and so the last bit) is not reproducible, like torch's scatter_add_ on a GPU; ACC = AccumFixed: push_accum.h, where a
// contribution of exactly 0 adds the integer 0.  Fixed-point bound, G = 1: t is val times three signs, the mask (0 or 1)
// and a product of three weights 1 - t or t with t = g - floor(g) in [0, 1], so |t| <= |val| <= m.
template <typename ACC>
__global__ void linear_push3d(const float* __restrict__ inp, int Bi, int C, const float* __restrict__ grid, int Bg,
                              int64_t nin, GridDims<3> dims, GridOpts op, int B, typename ACC::Cell* __restrict__ out,
                              typename ACC::Aux aux) {
    const int64_t n = (int64_t)B * nin;
    const int64_t vol = dims.count();
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nin, grid, Bg, dims, op.extrap);
        const LinearNodes q = linear_nodes(p, dims, op);
        for (int c = 0; c < C; ++c) {
            const int64_t sin = (int64_t)(Bi == 1 ? 0 : p.b) * C + c;
            const float val = inp[sin * nin + p.v];
            typename ACC::Cell* dst = out + ((int64_t)p.b * C + c) * vol;
            const auto scale = ACC::scale(aux, sin);
            if (ACC::dead(scale)) continue;
            LINEAR_CORNERS(a, bb, d) {
                float t = val * (float)(q.sg[0][a] * q.sg[1][bb] * q.sg[2][d]);
                t = t * p.mask;
                t = t * ((q.w[0][a] * q.w[1][bb]) * q.w[2][d]);
                ACC::add(dst + linear_offset(q, dims, a, bb, d), t, scale);
            }
        }
    }
}

// iso1.grad3d (iso1.py:268-387): spatial gradient of the trilinear interpolant at the grid coordinates, out
// [B][C][nout][3]
__global__ void linear_grad3d(const float* __restrict__ inp, int Bi, int C, GridDims<3> dims,
                              const float* __restrict__ grid, int Bg, int64_t nout, GridOpts op, int B,
                              float* __restrict__ out) {
    const int64_t n = (int64_t)B * nout;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, dims, op.extrap);
        const LinearNodes q = linear_nodes(p, dims, op);
        const float slope[2] = {-1.f, 1.f};
        const int64_t vol = dims.count();
        for (int c = 0; c < C; ++c) {
            const float* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            float ax = 0.f, ay = 0.f, az = 0.f;
            LINEAR_CORNERS(a, bb, d) {
                float val = ld_tex(src + linear_offset(q, dims, a, bb, d));
                val = val * (float)(q.sg[0][a] * q.sg[1][bb] * q.sg[2][d]);
                ax = fmaf(val, slope[a] * (q.w[1][bb] * q.w[2][d]), ax);
                ay = fmaf(val, slope[bb] * (q.w[0][a] * q.w[2][d]), ay);
                az = fmaf(val, slope[d] * (q.w[0][a] * q.w[1][bb]), az);
            }
            float* o = out + (((int64_t)p.b * C + c) * nout + p.v) * 3;
            o[0] = ax * p.mask; o[1] = ay * p.mask; o[2] = az * p.mask;
        }
    }
}

}  // namespace

// One launch of the family: `kernel` over n points
template <typename K, typename... A>
static int launch_grid(K kernel, int64_t n, bfm_stream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, bfm_s(stream), args...);
    return bfm_launch_status();
}

// The orders that have their own instantiation: 0, 2, 3 in 3-D, 0 to 3 in 2-D; any other call runs the padded one.
// go(std::integral_constant<int, O>) launches it.
template <int D, typename F>
static int launch_order(const GridOpts& op, F&& go) {
    int rc = BFM_OK;
    if constexpr (D == 3) dispatch_order<0, 2, 3>(op.order, [&](auto o) { rc = go(o); });
    else dispatch_order<0, 1, 2, 3>(op.order, [&](auto o) { rc = go(o); });
    return rc;
}

// pull and grad: image `in`, grid `og`.  LINEAR: the iso1 kernels, which take no orders.
template <int D, bool LINEAR, bool GRAD>
static int launch_sample(const float* inp, int Bi, int C, GridDims<D> in, const float* grid, int Bg, GridDims<D> og,
                         const int* bound, const int* order, int extrapolate, float* out, bfm_stream_t stream) {
    const int rc = grid_check_args(D, inp, grid, out, bound, order, Bi, Bg, C, in.n, og.n, extrapolate);
    if (rc != BFM_OK) return rc;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = og.count();
    const GridOpts op = grid_opts(D, bound, order, extrapolate);
    auto go = [&](auto kernel) { return launch_grid(kernel, B * nout, stream, inp, Bi, C, in, grid, Bg, nout, op, B, out); };
    if constexpr (LINEAR) return go(GRAD ? linear_grad3d : linear_pull3d);
    else return launch_order<D>(op, [&](auto o) {
        constexpr int O = decltype(o)::value;
        if constexpr (D == 3 && O < 0)
            return launch_grid(GRAD ? padded_grad3d : padded_pull3d, B * nout, stream, inp, Bi, C, in.n[0], in.n[1], in.n[2],
                               grid, Bg, nout, op, B, out);
        else return go(GRAD ? spline_grad<D, O> : spline_pull<D, O>);
    });
}

// push: source and grid `in`, volume `vol`, accumulated by the policy ACC (push_accum.h) in `acc`, zero on entry
template <int D, bool LINEAR, typename ACC>
static int launch_push(const float* inp, int Bi, int C, GridDims<D> in, const float* grid, int Bg, GridDims<D> vol,
                       const int* bound, const int* order, int extrapolate, typename ACC::Cell* acc, typename ACC::Aux aux,
                       bfm_stream_t stream) {
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nin = in.count();
    const GridOpts op = grid_opts(D, bound, order, extrapolate);
    auto go = [&](auto kernel) {
        return launch_grid(kernel, B * nin, stream, inp, Bi, C, grid, Bg, nin, vol, op, B, acc, aux);
    };
    if constexpr (LINEAR) return go(linear_push3d<ACC>);
    else return launch_order<D>(op, [&](auto o) {
        constexpr int O = decltype(o)::value;
        if constexpr (D == 3 && O < 0)
            return launch_grid(padded_push3d<ACC>, B * nin, stream, inp, Bi, C, grid, Bg, nin, vol.n[0], vol.n[1], vol.n[2],
                               op, B, acc, aux);
        else return go(spline_push<D, O, ACC>);
    });
}

// the float-atomic route: out_zeroed is the accumulator
template <int D, bool LINEAR>
static int push_atomic(const float* inp, int Bi, int C, GridDims<D> in, const float* grid, int Bg, GridDims<D> vol,
                       const int* bound, const int* order, int extrapolate, float* out_zeroed, bfm_stream_t stream) {
    const int rc = grid_check_args(D, inp, grid, out_zeroed, bound, order, Bi, Bg, C, in.n, vol.n, extrapolate);
    if (rc != BFM_OK) return rc;
    return launch_push<D, LINEAR, AccumFloat>(inp, Bi, C, in, grid, Bg, vol, bound, order, extrapolate, out_zeroed, {},
                                              stream);
}

// the fixed-point route: the maxima and exponents of the slices, the push into the int64 accumulators of the workspace,
// the conversion into out (push_fixed.hip).  P = the points of a batch item, T = the product of order + 1, G = 1.
template <int D, bool LINEAR>
static int push_fixed(const float* inp, int Bi, int C, GridDims<D> in, const float* grid, int Bg, GridDims<D> vol,
                      const int* bound, const int* order, int extrapolate, float* out, void* workspace,
                      size_t workspace_bytes, bfm_stream_t stream) {
    int rc = grid_check_args(D, inp, grid, out, bound, order, Bi, Bg, C, in.n, vol.n, extrapolate);
    if (rc != BFM_OK) return rc;
    PushFixedPlan plan;
    rc = push_fixed_begin(&plan, inp, Bi, C, in.count(), Bi > Bg ? Bi : Bg, vol.count(), in.count(), order, D, 1, workspace,
                          workspace_bytes, stream);
    if (rc != BFM_OK) return rc;
    rc = launch_push<D, LINEAR, AccumFixed>(inp, Bi, C, in, grid, Bg, vol, bound, order, extrapolate, plan.acc, plan.k,
                                            stream);
    return rc != BFM_OK ? rc : push_fixed_end(plan, out, stream);
}

extern "C" int bfm_grid_pull3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, const int* order,
                                      int extrapolate, float* out, bfm_stream_t stream) {
    return launch_sample<3, false, false>(inp, Bi, C, {{nx, ny, nz}}, grid, Bg, {{ox, oy, oz}}, bound, order, extrapolate,
                                          out, stream);
}

extern "C" int bfm_grid_push3d_spline(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                      int nx, int ny, int nz, const int* bound, const int* order, int extrapolate,
                                      float* out_zeroed, bfm_stream_t stream) {
    return push_atomic<3, false>(inp, Bi, C, {{ix, iy, iz}}, grid, Bg, {{nx, ny, nz}}, bound, order, extrapolate,
                                 out_zeroed, stream);
}

extern "C" int bfm_grid_grad3d_spline(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, const int* order,
                                      int extrapolate, float* out, bfm_stream_t stream) {
    return launch_sample<3, false, true>(inp, Bi, C, {{nx, ny, nz}}, grid, Bg, {{ox, oy, oz}}, bound, order, extrapolate,
                                         out, stream);
}

extern "C" int bfm_grid_pull2d_spline(const float* inp, int Bi, int C, int nx, int ny, const float* grid, int Bg, int ox,
                                      int oy, const int* bound, const int* order, int extrapolate, float* out,
                                      bfm_stream_t stream) {
    return launch_sample<2, false, false>(inp, Bi, C, {{nx, ny}}, grid, Bg, {{ox, oy}}, bound, order, extrapolate, out,
                                          stream);
}

extern "C" int bfm_grid_push2d_spline(const float* inp, int Bi, int C, int ix, int iy, const float* grid, int Bg, int nx,
                                      int ny, const int* bound, const int* order, int extrapolate, float* out_zeroed,
                                      bfm_stream_t stream) {
    return push_atomic<2, false>(inp, Bi, C, {{ix, iy}}, grid, Bg, {{nx, ny}}, bound, order, extrapolate, out_zeroed,
                                 stream);
}

extern "C" int bfm_grid_grad2d_spline(const float* inp, int Bi, int C, int nx, int ny, const float* grid, int Bg, int ox,
                                      int oy, const int* bound, const int* order, int extrapolate, float* out,
                                      bfm_stream_t stream) {
    return launch_sample<2, false, true>(inp, Bi, C, {{nx, ny}}, grid, Bg, {{ox, oy}}, bound, order, extrapolate, out,
                                         stream);
}

extern "C" int bfm_grid_pull3d_linear(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, int extrapolate, float* out,
                                      bfm_stream_t stream) {
    return launch_sample<3, true, false>(inp, Bi, C, {{nx, ny, nz}}, grid, Bg, {{ox, oy, oz}}, bound, GRID_LINEAR,
                                         extrapolate, out, stream);
}

extern "C" int bfm_grid_push3d_linear(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid, int Bg,
                                      int nx, int ny, int nz, const int* bound, int extrapolate, float* out_zeroed,
                                      bfm_stream_t stream) {
    return push_atomic<3, true>(inp, Bi, C, {{ix, iy, iz}}, grid, Bg, {{nx, ny, nz}}, bound, GRID_LINEAR, extrapolate,
                                out_zeroed, stream);
}

extern "C" int bfm_grid_grad3d_linear(const float* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                                      int Bg, int ox, int oy, int oz, const int* bound, int extrapolate, float* out,
                                      bfm_stream_t stream) {
    return launch_sample<3, true, true>(inp, Bi, C, {{nx, ny, nz}}, grid, Bg, {{ox, oy, oz}}, bound, GRID_LINEAR,
                                        extrapolate, out, stream);
}

extern "C" int bfm_grid_push3d_spline_fixed(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid,
                                            int Bg, int nx, int ny, int nz, const int* bound, const int* order,
                                            int extrapolate, float* out, void* workspace, size_t workspace_bytes,
                                            bfm_stream_t stream) {
    return push_fixed<3, false>(inp, Bi, C, {{ix, iy, iz}}, grid, Bg, {{nx, ny, nz}}, bound, order, extrapolate, out,
                                workspace, workspace_bytes, stream);
}

extern "C" int bfm_grid_push2d_spline_fixed(const float* inp, int Bi, int C, int ix, int iy, const float* grid, int Bg,
                                            int nx, int ny, const int* bound, const int* order, int extrapolate, float* out,
                                            void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    return push_fixed<2, false>(inp, Bi, C, {{ix, iy}}, grid, Bg, {{nx, ny}}, bound, order, extrapolate, out, workspace,
                                workspace_bytes, stream);
}

extern "C" int bfm_grid_push3d_linear_fixed(const float* inp, int Bi, int C, int ix, int iy, int iz, const float* grid,
                                            int Bg, int nx, int ny, int nz, const int* bound, int extrapolate, float* out,
                                            void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    return push_fixed<3, true>(inp, Bi, C, {{ix, iy, iz}}, grid, Bg, {{nx, ny, nz}}, bound, GRID_LINEAR, extrapolate, out,
                               workspace, workspace_bytes, stream);
}
