// The element-wise half of a hidden task-head layer (Trainer/models/head.py:27-31,52-55,152-167: ConvBlock =
// Conv3d(3, padding 1, bias) + LeakyReLU(0.2), no GroupNorm).  The convolution itself runs on the existing conv kernels
// with the identity affine and slope 1 (the data-gradient convolutions' form); these kernels add what those lack:
//   forward   y = lrelu(y + b[c]) in place, and max |y| -- the next hidden layer's prescale bound -- in the same pass
//   backward  dP = dY * lrelu'(Y), max |dP| (the weight-gradient kernel's bound) and dbias[c] = sum_v dP[v][c] in one pass
// Channels-last fp32, C % 4 == 0, 16-byte accesses.  The maxima fold by an integer atomic maximum of the bit pattern (any
// order gives the same bits); dbias goes through fixed-order fp64 partials, no atomics.
#include "bfm_common.h"

namespace {

constexpr int HL_THREADS = 256;
constexpr int HL_MAX_BLOCKS = 1024;

__device__ __forceinline__ float hl_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float hl_max4(float4 v) {
    return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// block maximum -> one atomic per block
__device__ __forceinline__ void hl_fold_max(float m, unsigned* out) {
    m = wave_reduce_max(m);
    __shared__ float red[HL_THREADS / BFM_WAVE];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = red[0];
#pragma unroll
        for (int i = 1; i < HL_THREADS / BFM_WAVE; ++i) r = fmaxf(r, red[i]);
        atomicMax(out, __float_as_uint(r));
    }
}

// q = C / 4 float4 columns per voxel; element i of the float4 view belongs to voxel i / q, column i % q.  The grid's
// stride keeps a thread's column walk in 32-bit arithmetic.  mask (or NULL): voxels whose mask value is zero are left as
// they are and take no part in the maximum (the masked convolution leaves whole boxes of them unwritten).
__global__ void __launch_bounds__(HL_THREADS) bias_lrelu_kernel(float4* __restrict__ y, const float4* __restrict__ bias, int q,
                                                                int64_t n4, float slope, const float* __restrict__ mask,
                                                                unsigned* __restrict__ bound) {
    const int64_t stride = (int64_t)gridDim.x * HL_THREADS;
    const int step = (int)(stride % q);
    int64_t i = (int64_t)blockIdx.x * HL_THREADS + threadIdx.x;
    int c = (int)(i % q);
    float m = 0.f;
    for (; i < n4; i += stride) {
        if (!mask || mask[i / q] != 0.f) {
            const float4 v = y[i], b = bias[c];
            const float4 r = make_float4(hl_lrelu(v.x + b.x, slope), hl_lrelu(v.y + b.y, slope), hl_lrelu(v.z + b.z, slope),
                                         hl_lrelu(v.w + b.w, slope));
            y[i] = r;
            m = fmaxf(m, hl_max4(r));
        }
        c += step;
        if (c >= q) c -= q;
    }
    if (bound) hl_fold_max(m, bound);
}

// Block b owns the voxels [b * chunk, (b + 1) * chunk).  Thread t: column t % q, voxel row t / q of every R = 256 / q
// voxels (threads beyond R * q idle).  Per thread an fp64 sum of its rows in ascending order; the block folds its R rows in
// ascending order into partial[b][C]; hl_fold_partials folds the blocks in ascending order.
__global__ void __launch_bounds__(HL_THREADS) bias_lrelu_bwd_kernel(const float4* __restrict__ dY, const float4* __restrict__ Y,
                                                                    int q, int64_t nvox, int64_t chunk, float slope,
                                                                    float4* __restrict__ dP, double* __restrict__ partial,
                                                                    unsigned* __restrict__ absmax) {
    extern __shared__ double hl_sm[];                           // [R][4 q]
    const int R = HL_THREADS / q;
    const int col = threadIdx.x % q, row = threadIdx.x / q;
    const int64_t v0 = (int64_t)blockIdx.x * chunk;
    const int64_t v1 = v0 + chunk < nvox ? v0 + chunk : nvox;
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
    float m = 0.f;
    if (row < R) {
        for (int64_t v = v0 + row; v < v1; v += R) {
            const int64_t i = v * q + col;
            const float4 g = dY[i], o = Y[i];
            const float4 p = make_float4(g.x * (o.x > 0.f ? 1.f : slope), g.y * (o.y > 0.f ? 1.f : slope),
                                         g.z * (o.z > 0.f ? 1.f : slope), g.w * (o.w > 0.f ? 1.f : slope));
            dP[i] = p;
            s0 += (double)p.x; s1 += (double)p.y; s2 += (double)p.z; s3 += (double)p.w;
            m = fmaxf(m, hl_max4(p));
        }
        double* d = hl_sm + ((size_t)row * q + col) * 4;
        d[0] = s0; d[1] = s1; d[2] = s2; d[3] = s3;
    }
    __syncthreads();
    const int C = 4 * q;
    for (int c = threadIdx.x; c < C; c += HL_THREADS) {
        double s = 0.;
        for (int r = 0; r < R; ++r) s += hl_sm[(size_t)r * C + c];
        partial[(size_t)blockIdx.x * C + c] = s;
    }
    if (absmax) hl_fold_max(m, absmax);
}

__global__ void hl_fold_partials(const double* __restrict__ partial, int nblocks, int C, float* __restrict__ dbias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.;
    for (int b = 0; b < nblocks; ++b) s += partial[(size_t)b * C + c];
    dbias[c] = (float)s;
}

inline bool hl_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blocks of the backward pass: a function of the voxel count alone (the partials' order is part of the result's bits)
inline int hl_bwd_blocks(int64_t nvox) {
    const int64_t b = bfm_cdiv64(nvox, 256);
    return (int)(b < 1 ? 1 : (b > HL_MAX_BLOCKS ? HL_MAX_BLOCKS : b));
}

}  // namespace

extern "C" int bfm_head_bias_lrelu(float* y, const float* bias, int C, int64_t nvox, float slope, const float* mask_image,
                                   float* bound_out, bfm_stream_t stream) {
    if (!y || !bias || C <= 0 || nvox <= 0) return BFM_E_ARG;
    if (C % 4 || !hl_aligned16(y) || !hl_aligned16(bias)) return BFM_E_SHAPE;
    const int q = C / 4;
    const int64_t n4 = nvox * q;
    if (bound_out && hipMemsetAsync(bound_out, 0, sizeof(float), bfm_s(stream)) != hipSuccess) return BFM_E_LAUNCH;
    const int64_t nb = bfm_cdiv64(n4, HL_THREADS);
    const int grid = (int)(nb > 4096 ? 4096 : nb);
    hipLaunchKernelGGL(bias_lrelu_kernel, dim3(grid), dim3(HL_THREADS), 0, bfm_s(stream), reinterpret_cast<float4*>(y),
                       reinterpret_cast<const float4*>(bias), q, n4, slope, mask_image, reinterpret_cast<unsigned*>(bound_out));
    return bfm_launch_status();
}

extern "C" size_t bfm_head_bias_lrelu_bwd_workspace(int C, int64_t nvox) {
    if (C <= 0 || nvox <= 0) return 0;
    return (size_t)hl_bwd_blocks(nvox) * C * sizeof(double);
}

extern "C" int bfm_head_bias_lrelu_bwd(const float* dY, const float* Y, int C, int64_t nvox, float slope, float* dP,
                                       float* dbias, float* absmax_out, void* workspace, size_t workspace_bytes,
                                       bfm_stream_t stream) {
    if (!dY || !Y || !dP || !dbias || !workspace || C <= 0 || nvox <= 0) return BFM_E_ARG;
    if (C % 4 || C / 4 > HL_THREADS || !hl_aligned16(dY) || !hl_aligned16(Y) || !hl_aligned16(dP)) return BFM_E_SHAPE;
    if (workspace_bytes < bfm_head_bias_lrelu_bwd_workspace(C, nvox) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return BFM_E_WORKSPACE;
    const int q = C / 4, R = HL_THREADS / q;
    const int nblocks = hl_bwd_blocks(nvox);
    const int64_t chunk = bfm_cdiv64(nvox, nblocks);
    if (absmax_out && hipMemsetAsync(absmax_out, 0, sizeof(float), bfm_s(stream)) != hipSuccess) return BFM_E_LAUNCH;
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(bias_lrelu_bwd_kernel, dim3(nblocks), dim3(HL_THREADS), (size_t)R * C * sizeof(double), bfm_s(stream),
                       reinterpret_cast<const float4*>(dY), reinterpret_cast<const float4*>(Y), q, nvox, chunk, slope,
                       reinterpret_cast<float4*>(dP), partial, reinterpret_cast<unsigned*>(absmax_out));
    hipLaunchKernelGGL(hl_fold_partials, dim3(bfm_cdiv(C, 64)), dim3(64), 0, bfm_s(stream), partial, nblocks, C, dbias);
    return bfm_launch_status();
}
