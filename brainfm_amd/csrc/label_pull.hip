// interpol.grid_pull on an integer image: the label branch of the vendored torch-interpol (utils/interpol/api.py:182-193).
// The reference pulls the indicator of every label of unique() and keeps, per output voxel, the label whose interpolated
// weight is the largest (strict >, labels in ascending order, so the smallest label wins a tie; 0 where no weight is
// positive).  The weight of a label at a voxel is the sum, over the taps of the voxel's footprint that hold the label, of
// the separable spline weight times the bound sign -- it depends on the at most 64 taps only.  So: one pass, one thread per
// output voxel, prologue and nodes / signs / weights (grid_kernels.h, spline_nodes.h) those of spline_grid.hip, the labels of the
// footprint gathered with ld_tex loads of the label's own width (an int64 label as two 4-byte halves), and the per-label
// sums and the winner formed inside the thread.  No one-hot, no per-label volume, no unique(): the cost does not depend on
// the number of labels of the image.
//
// Sums are fp32, the weight of a tap is ((wx * wy) * wz) * mask as in spline_pull3d, and the taps of a label are added in
// the fixed tap order (x slowest): the result is the same bits from run to run, and two labels with the same weights at
// the same relative taps get the same sum.
//
// Three ways to keep the (label, sum) table, since a table indexed by a run-time value would go to scratch:
//   regs    the footprint's labels and weights stay in registers (constant indices only) and every tap rescans the
//           footprint for its own label: T^2 compare-and-add for T taps.  AUTO takes it for the all-nearest and all-linear
//           footprints (1 and 8 taps).
//   passes  four (label, sum) slots in registers hold the four smallest labels not done yet; a footprint with more
//           distinct labels is walked again (label_pull3d_passes below).  AUTO takes it for 27 and 64 taps (64 also for
//           mixed orders, whose unused taps have the weight 0 and are skipped): on a segmentation nearly every footprint
//           is done in one pass, at the cost of the float pull of the same order.
//   lds     a slice of LDS per thread, entry e of lane l at [e * 64 + l] (conflict-free); every tap with a non-zero weight
//           looks its label up among the entries so far and adds to it or appends: T x (distinct labels) steps, one wave
//           per block, nothing synchronised.  32 KB per wave at 64 taps: five waves per CU, which is what makes it 2.9
//           times slower than `passes` on a segmentation.  With one random label per voxel (about 45 distinct labels in a
//           cubic footprint, 12 passes) it is still 1.9 times slower at 64 taps and 0.82 times as slow at 27.
// `variant` of the export forces one for measurements (scripts/bench_label_pull.py, profiles/label_pull.txt, where the
// choice of AUTO comes from).  All give the same bits.
#include "grid_kernels.h"

namespace {

// label loads under the texel policy of gather3d.h (agent scope: past the vector L1); K is the type labels are compared in
template <typename LT> struct Key { typedef int32_t type; };
template <> struct Key<int64_t> { typedef int64_t type; };

__device__ __forceinline__ int32_t ld_label(const uint8_t* p) {
    return (int32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t ld_label(const int16_t* p) {
    return (int32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t ld_label(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int64_t ld_label(const int64_t* p) {
    const uint32_t* h = reinterpret_cast<const uint32_t*>(p);
    const uint32_t lo = ld_tex(h), hi = ld_tex(h + 1);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// O = 0, 1, 2, 3: isotropic order O with O + 1 taps per axis; O < 0: per-axis orders from `op`, 4 taps per axis
template <int O, typename LT>
__global__ void __launch_bounds__(256) label_pull3d_regs(const LT* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                         const float* __restrict__ grid, int Bg, int64_t nout,
                                                         GridOpts op, int B, LT* __restrict__ out) {
    typedef typename Key<LT>::type K;
    constexpr int T = grid_taps(O), N = T * T * T;
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
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
            LT* dst = out + ((int64_t)p.b * C + c) * nout + p.v;
            if (p.mask == 0.f) { *dst = (LT)0; continue; }
            const LT* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            K lab[N];
            float w[N];
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const LT* row = src + ((int64_t)ix[a] * ny + iy[bb]) * nz;
                    const float wxy = wx[a] * wy[bb];
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        lab[(a * T + bb) * T + d] = ld_label(row + iz[d]);
                        w[(a * T + bb) * T + d] = wxy * wz[d];
                    }
                }
            K best_l = 0;
            float best = 0.f;
#pragma unroll
            for (int p = 0; p < N; ++p) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < N; ++q) s += lab[q] == lab[p] ? w[q] : 0.f;
                if (s > best || (s == best && s > 0.f && lab[p] < best_l)) { best = s; best_l = lab[p]; }
            }
            *dst = (LT)best_l;
        }
    }
}

template <int O, typename LT>
__global__ void __launch_bounds__(64) label_pull3d_lds(const LT* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                       const float* __restrict__ grid, int Bg, int64_t nout,
                                                       GridOpts op, int B, LT* __restrict__ out) {
    typedef typename Key<LT>::type K;
    constexpr int T = grid_taps(O), N = T * T * T;
    __shared__ K keys[N * 64];
    __shared__ float sums[N * 64];
    const int lane = threadIdx.x;
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        int iy[T], iz[T];                                          // the x nodes: axis_node, slab by slab
        float wy[T], wz[T];
        axis_nodes<T>(p.g[1], oy, ny, op.bound[1], iy, wy);
        axis_nodes<T>(p.g[2], oz, nz, op.bound[2], iz, wz);
        for (int c = 0; c < C; ++c) {
            LT* dst = out + ((int64_t)p.b * C + c) * nout + p.v;
            if (p.mask == 0.f) { *dst = (LT)0; continue; }
            const LT* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            int cnt = 0;                                           // entries of this thread's table, at most N
#pragma unroll 1
            for (int a = 0; a < T; ++a) {                          // rolled: one x-slab of the footprint at a time
                int ixa;
                float wxa;
                axis_node(p.g[0], ox, nx, op.bound[0], a, ixa, wxa);
                K lab[T * T];                                      // its loads go out together
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const LT* row = src + ((int64_t)ixa * ny + iy[bb]) * nz;
#pragma unroll
                    for (int d = 0; d < T; ++d) lab[bb * T + d] = ld_label(row + iz[d]);
                }
#pragma unroll
                for (int bb = 0; bb < T; ++bb) {
                    const float wxy = wxa * wy[bb];
#pragma unroll
                    for (int d = 0; d < T; ++d) {
                        const float w = wxy * wz[d];
                        if (w == 0.f) continue;                    // adds nothing to any sum, and a sum of 0 never wins
                        const K l = lab[bb * T + d];
                        int e = 0;
                        while (e < cnt && keys[e * 64 + lane] != l) ++e;
                        if (e == cnt) {                            // cnt < N here: at most N taps get this far
                            keys[e * 64 + lane] = l;
                            sums[e * 64 + lane] = w;
                            ++cnt;
                        } else {
                            sums[e * 64 + lane] += w;
                        }
                    }
                }
            }
            K best_l = 0;
            float best = 0.f;
            for (int e = 0; e < cnt; ++e) {
                const float s = sums[e * 64 + lane];
                const K l = keys[e * 64 + lane];
                if (s > best || (s == best && s > 0.f && l < best_l)) { best = s; best_l = l; }
            }
            *dst = (LT)best_l;
        }
    }
}

// No table at all: S (label, sum) slots in registers hold the S smallest labels above `floor` that the pass has met, a
// tap whose label is not among them and is smaller than their largest evicts that one (whose taps so far are dropped: it
// is done again later), and a pass that had to evict or skip runs again with floor = the largest label it kept.  A label
// is only ever skipped for being larger than the current largest slot, which never grows during a pass, so a label that
// is in a slot at the end of a pass has had every one of its taps, in tap order.  ceil(distinct labels / S) passes over
// the footprint (whose labels the later passes read from the caches again): one for the footprints of a segmentation,
// 16 for the 64 distinct labels of the worst case.  Slots are addressed by constants (selects), never by a run-time index.
template <int O, typename LT>
__global__ void __launch_bounds__(256) label_pull3d_passes(const LT* __restrict__ inp, int Bi, int C, int nx, int ny, int nz,
                                                           const float* __restrict__ grid, int Bg, int64_t nout,
                                                           GridOpts op, int B, LT* __restrict__ out) {
    typedef typename Key<LT>::type K;
    constexpr int T = grid_taps(O), S = 4;
    const int ox = axis_order<O>(op, 0), oy = axis_order<O>(op, 1), oz = axis_order<O>(op, 2);
    const int64_t n = (int64_t)B * nout;
    const int64_t vol = (int64_t)nx * ny * nz;
    GRID_STRIDE(i, n) {
        const GridPoint<3> p = grid_point<3>(i, nout, grid, Bg, GridDims<3>{{nx, ny, nz}}, op.extrap);
        int iy[T], iz[T];                                          // the x nodes: axis_node, slab by slab
        float wy[T], wz[T];
        axis_nodes<T>(p.g[1], oy, ny, op.bound[1], iy, wy);
        axis_nodes<T>(p.g[2], oz, nz, op.bound[2], iz, wz);
        for (int c = 0; c < C; ++c) {
            LT* dst = out + ((int64_t)p.b * C + c) * nout + p.v;
            if (p.mask == 0.f) { *dst = (LT)0; continue; }
            const LT* src = inp + ((int64_t)(Bi == 1 ? 0 : p.b) * C + c) * vol;
            K best_l = 0;
            float best = 0.f;
            bool have_floor = false;
            K floor_l = 0;
            for (;;) {
                K key[S];
                float sum[S];
                int cnt = 0, top = 0;                              // slots in use; the slot of the largest key once full
                bool more = false;
#pragma unroll
                for (int s = 0; s < S; ++s) { key[s] = 0; sum[s] = 0.f; }
#pragma unroll 1
                for (int a = 0; a < T; ++a) {                      // rolled: one x-slab of the footprint at a time
                    int ixa;
                    float wxa;
                    axis_node(p.g[0], ox, nx, op.bound[0], a, ixa, wxa);
                    K lab[T * T];
#pragma unroll
                    for (int bb = 0; bb < T; ++bb) {
                        const LT* row = src + ((int64_t)ixa * ny + iy[bb]) * nz;
#pragma unroll
                        for (int d = 0; d < T; ++d) lab[bb * T + d] = ld_label(row + iz[d]);
                    }
#pragma unroll
                    for (int bb = 0; bb < T; ++bb) {
                        const float wxy = wxa * wy[bb];
#pragma unroll
                        for (int d = 0; d < T; ++d) {
                            const float w = wxy * wz[d];
                            const K l = lab[bb * T + d];
                            if (w == 0.f || (have_floor && l <= floor_l)) continue;
                            bool hit = false;
#pragma unroll
                            for (int s = 0; s < S; ++s)
                                if (s < cnt && key[s] == l) { sum[s] += w; hit = true; }
                            if (hit) continue;
                            K top_l = key[0];
#pragma unroll
                            for (int s = 1; s < S; ++s) top_l = top == s ? key[s] : top_l;
                            if (cnt == S) {
                                more = true;
                                if (l > top_l) continue;           // not among the S smallest: a later pass
                            }
                            const int pos = cnt < S ? cnt : top;
#pragma unroll
                            for (int s = 0; s < S; ++s)
                                if (s == pos) { key[s] = l; sum[s] = w; }
                            cnt = cnt < S ? cnt + 1 : S;
                            if (cnt == S) {                        // where the largest key sits now
                                top = 0;
                                K m = key[0];
#pragma unroll
                                for (int s = 1; s < S; ++s)
                                    if (key[s] > m) { m = key[s]; top = s; }
                            }
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (s < cnt && (sum[s] > best || (sum[s] == best && sum[s] > 0.f && key[s] < best_l))) {
                        best = sum[s];
                        best_l = key[s];
                    }
                }
                if (!more) break;
                K m = key[0];
#pragma unroll
                for (int s = 1; s < S; ++s) m = key[s] > m ? key[s] : m;
                floor_l = m;
                have_floor = true;
            }
            *dst = (LT)best_l;
        }
    }
}

template <int O, typename LT>
void launch_one(int how, int64_t n, hipStream_t s, const LT* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                int Bg, int64_t nout, GridOpts op, int B, LT* out) {
    if (how == BFM_LABEL_PULL_LDS)
        hipLaunchKernelGGL((label_pull3d_lds<O, LT>), dim3(grid_for(n, 64, 32768)), dim3(64), 0, s, inp, Bi, C, nx, ny, nz, grid,
                           Bg, nout, op, B, out);
    else if (how == BFM_LABEL_PULL_REGS)
        hipLaunchKernelGGL((label_pull3d_regs<O, LT>), dim3(grid_for(n)), dim3(256), 0, s, inp, Bi, C, nx, ny, nz, grid, Bg,
                           nout, op, B, out);
    else
        hipLaunchKernelGGL((label_pull3d_passes<O, LT>), dim3(grid_for(n)), dim3(256), 0, s, inp, Bi, C, nx, ny, nz, grid, Bg,
                           nout, op, B, out);
}

// every isotropic order has its own instantiation; AUTO: regs for 1 and 8 taps, passes for 27 and 64
template <typename LT>
void launch_dtype(int variant, hipStream_t s, const void* inp, int Bi, int C, int nx, int ny, int nz, const float* grid,
                  int Bg, int64_t nout, GridOpts op, int B, void* out) {
    dispatch_order<0, 1, 2, 3>(op.order, [&](auto o) {
        constexpr int O = decltype(o)::value;
        const int how = variant != BFM_LABEL_PULL_AUTO ? variant
                                                       : ((O == 0 || O == 1) ? BFM_LABEL_PULL_REGS : BFM_LABEL_PULL_PASSES);
        launch_one<O, LT>(how, B * nout, s, static_cast<const LT*>(inp), Bi, C, nx, ny, nz, grid, Bg, nout, op, B,
                          static_cast<LT*>(out));
    });
}

}  // namespace

extern "C" int bfm_label_pull3d(const void* inp, int dtype, int Bi, int C, int nx, int ny, int nz, const float* grid, int Bg,
                                int ox, int oy, int oz, const int* bound, const int* order, int extrapolate, int variant,
                                void* out, bfm_stream_t stream) {
    const GridDims<3> in{{nx, ny, nz}}, og{{ox, oy, oz}};
    const int rc = grid_check_args(3, inp, grid, out, bound, order, Bi, Bg, C, in.n, og.n, extrapolate);
    if (rc != BFM_OK) return rc;
    if (dtype < BFM_LABEL_U8 || dtype > BFM_LABEL_I64) return BFM_E_ARG;
    if (variant < BFM_LABEL_PULL_AUTO || variant > BFM_LABEL_PULL_PASSES) return BFM_E_ARG;
    const int B = Bi > Bg ? Bi : Bg;
    const int64_t nout = og.count();
    const GridOpts op = grid_opts(3, bound, order, extrapolate);
    hipStream_t s = bfm_s(stream);
    switch (dtype) {
        case BFM_LABEL_U8: launch_dtype<uint8_t>(variant, s, inp, Bi, C, nx, ny, nz, grid, Bg, nout, op, B, out); break;
        case BFM_LABEL_I16: launch_dtype<int16_t>(variant, s, inp, Bi, C, nx, ny, nz, grid, Bg, nout, op, B, out); break;
        case BFM_LABEL_I32: launch_dtype<int32_t>(variant, s, inp, Bi, C, nx, ny, nz, grid, Bg, nout, op, B, out); break;
        default: launch_dtype<int64_t>(variant, s, inp, Bi, C, nx, ny, nz, grid, Bg, nout, op, B, out); break;
    }
    return bfm_launch_status();
}
