// What conv3d_wino.hip (F(2,3)) and conv3d_wino4.hip (F(4,3)) share: the box of a volume, the device-built lists of the
// boxes a sparse launch computes -- the flags of bfm_uniform_boxes and the lists of both kernels are per box, so both
// kernels must cut a volume into the same boxes -- and the arguments and first checks of their launchers.
#pragma once
#include "conv_shared.h"

// the 256-voxel box (TD x TH x TW) conv_wino uses for this volume; false: none fits
bool bfm_wino_choose_box(int D, int H, int W, int npl, int& TD, int& TH, int& TW);

__host__ __device__ static inline size_t bfm_pad4(size_t n) { return (n + 3) & ~(size_t)3; }

// The masked forms' workspace of a volume of n boxes: act[n pad 4] | count | list[n]
// (wino_box_active_kernel / wino_mask_list_kernel: the boxes that hold a non-zero voxel of the mask image, ascending).
struct MaskListBuf {
    void* ws;
    size_t n;
    static size_t bytes(size_t n) { return bfm_pad4(n) + 4 + n * 4; }
    unsigned char* act() const { return static_cast<unsigned char*>(ws); }
    int* count() const { return reinterpret_cast<int*>(act() + bfm_pad4(n)); }
    int* list() const { return count() + 1; }
};

// The flag buffer of bfm_uniform_boxes for a volume of n boxes:
//   flags[n pad 4] | first[27] | counts[2] | rest list[n] | uniform list[n] | need count | need list[n] | need[n pad 4]
// flags: 0, or 1 + class; first: the first flagged box of each class (n: none); counts / lists (uniform_lists_kernel):
// the unflagged boxes and every class's first box (the _rest kernels), then the other flagged boxes (the _uniform ones).
// need[b] = 1 for a class mate (flagged, not its class's first box) with a computed box -- unflagged, or a class's first --
// among its up to 26 neighbours in the grid, else 0; need list: those mates, ascending.  A computed box stages its input
// with a one-voxel halo, so of a tensor that only the _rest / _uniform pair on THESE flags reads, the mates without `need`
// are never read: a producer launched "by need" (bit 1 of its flag argument) leaves them unwritten.
struct UniformFlagBuf {
    const unsigned char* flags;
    size_t n;
    static size_t bytes(size_t n) { return bfm_pad4(n) + 27 * 4 + 2 * 4 + 2 * n * 4 + 4 + n * 4 + bfm_pad4(n); }
    __host__ __device__ int* first() const { return reinterpret_cast<int*>(const_cast<unsigned char*>(flags) + bfm_pad4(n)); }
    __host__ __device__ int* counts() const { return first() + 27; }
    __host__ __device__ int* rest_list() const { return counts() + 2; }
    __host__ __device__ int* uniform_list() const { return rest_list() + n; }
    __host__ __device__ int* need_count() const { return uniform_list() + n; }
    __host__ __device__ int* need_list() const { return need_count() + 1; }
    __host__ __device__ unsigned char* need() const { return reinterpret_cast<unsigned char*>(need_list() + n); }
};

// builds MaskListBuf{ws, nMt} on the stream; returns the launch status
int bfm_wino_mask_list(const float* mask_img, int D, int H, int W, int TD, int TH, int TW, int nTy, int nTx, int nMt, void* ws,
                       bfm_stream_t stream);

// One launch of either family, as the extern "C" entry points hand it to wino_launch / w4_launch.
struct WinoLaunch {
    const float* A;
    int CA, D, H, W;
    const float *scale, *shift, *bound;
    int G;
    const void* wpacked;
    int wexp, Cout;
    float slope;
    int passes, flags;
    float* out;
    void* moment_rows;
    bfm_stream_t stream;
    struct { const float* img = nullptr; void* ws = nullptr; } mask;               // the boxes that hold input only
    struct { const unsigned char* flags = nullptr; float* scratch = nullptr; const float* keep = nullptr; } uniform;   // the _rest / _uniform pair
    struct { float* out = nullptr; void* rows = nullptr; } pool;                   // F(2,3): fused MaxPool3d(2)
    struct { int S = 1, affine_stride = 0; } batch;                                // F(4,3): S same-shape samples
};

// The checks both launchers start with, in the order that decides which code a call with two faults returns.
static inline int bfm_wino_check(const WinoLaunch& a, int KC) {
    // bit 0 = accumulate; bit 1 (the _rest / _uniform pair only) = class mates are stored by need; nothing else is defined
    if (a.flags & ~(a.uniform.flags ? 3 : 1)) return BFM_E_ARG;
    if (!a.A || a.CA <= 0 || a.D <= 0 || a.H <= 0 || a.W <= 0 || !a.scale || !a.shift || !a.bound || a.G <= 0 || !a.wpacked ||
        !a.out)
        return BFM_E_ARG;
    if (a.CA % KC || a.Cout % 64 || a.Cout <= 0) return BFM_E_SHAPE;
    if (a.passes != 1 && a.passes != 3) return BFM_E_ARG;
    if ((reinterpret_cast<uintptr_t>(a.A) & 15) || (reinterpret_cast<uintptr_t>(a.scale) & 15) ||
        (reinterpret_cast<uintptr_t>(a.shift) & 15) || (reinterpret_cast<uintptr_t>(a.wpacked) & 15) ||
        (reinterpret_cast<uintptr_t>(a.out) & 15))
        return BFM_E_ARG;
    if ((int64_t)a.D * a.H * a.W * a.CA > 0x7fffffffLL) return BFM_E_SHAPE;       // 32-bit staging offsets
    return BFM_OK;
}
