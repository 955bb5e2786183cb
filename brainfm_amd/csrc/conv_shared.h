// What the convolution sources (conv3d_direct / _mfma / _upfold / _wino / _wino4) share: the lane -> row order of the MFMA
// operand reads and the host-side pieces every launcher needs (moment-row view, K<3> / K<1> by `passes`, the dynamic-LDS
// limit, the box count of a volume).  The epilogues' moment-row fold is NOT here: as a shared inline function it changed
// the instruction stream of every Winograd kernel (register allocation around the fold), so each body keeps its copy.  Host helpers are static inline and
// allocate nothing: the training path is host-paced.
#pragma once
#include "bfm_common.h"
#include <initializer_list>

// lane (= MFMA row) -> position inside the 32-row block such that every ds_read_b128 lane group {0-3,12-15,20-27} /
// {4-11,16-19,28-31} reads 16 consecutive box positions (one w-run when TW == 16): conflict-free
__device__ __forceinline__ int row_perm(int l) {
    if (l < 4) return l;
    if (l < 12) return l + 12;
    if (l < 16) return l - 8;
    if (l < 20) return l + 8;
    if (l < 28) return l - 12;
    return l;
}

__device__ __forceinline__ int row_unperm(int q) {      // inverse of row_perm
    if (q < 4) return q;
    if (q < 8) return q + 8;
    if (q < 16) return q + 12;
    if (q < 24) return q - 12;
    if (q < 28) return q - 8;
    return q;
}

// The four tables of a moment-row buffer of n values each: {sum, sumsq} fp64, then {min, max} fp32.
struct MomentRows {
    double *rsum = nullptr, *rsq = nullptr;
    float *rmn = nullptr, *rmx = nullptr;
    bool carve(void* rows, size_t n) {                           // false: `rows` is not 8-byte aligned
        if (reinterpret_cast<uintptr_t>(rows) & 7) return false;
        char* rb = static_cast<char*>(rows);
        rsum = reinterpret_cast<double*>(rb);
        rsq = reinterpret_cast<double*>(rb + n * 8);
        rmn = reinterpret_cast<float*>(rb + n * 16);
        rmx = reinterpret_cast<float*>(rb + n * 20);
        return true;
    }
    template <class P>
    void into(P& p) const { p.rsum = rsum; p.rsq = rsq; p.rmn = rmn; p.rmx = rmx; }
};

// the three-pass (split fp16) or the one-pass instance of a kernel, by `passes` (validated by the caller: 1 or 3)
template <class P>
static inline void bfm_launch_by_passes(int passes, void (*k3)(P), void (*k1)(P), dim3 grid, dim3 block, size_t smem,
                                        hipStream_t st, const P& p) {
    void (*k)(P) = passes == 3 ? k3 : k1;
    hipLaunchKernelGGL(k, grid, block, smem, st, p);
}

template <class F>
static inline const void* bfm_kernel(F* f) { return reinterpret_cast<const void*>(f); }

// Raise the dynamic-LDS limit of `kernels` to `bytes`, once per process (`done` is the caller's static flag); a failed
// attribute call is BFM_E_LAUNCH and is tried again by the next call.
static inline int bfm_raise_lds_limit(bool& done, std::initializer_list<const void*> kernels, int bytes) {
    if (done) return BFM_OK;
    for (const void* k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return BFM_E_LAUNCH;
    done = true;
    return BFM_OK;
}

// boxes of TD x TH x TW a (D,H,W) volume is cut into (the last ones along an axis may reach past it)
static inline int64_t bfm_box_count(int D, int H, int W, int TD, int TH, int TW) {
    return (int64_t)bfm_cdiv(D, TD) * bfm_cdiv(H, TH) * bfm_cdiv(W, TW);
}
