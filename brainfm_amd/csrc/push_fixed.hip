// The passes around a fixed-point grid_push / grid_pushgrad (push_accum.h): the maximum of every
// input slice, its exponent k, and the conversion of the int64 accumulators to fp32.  All on the device and on the call's
// stream: nothing is read back to the host.
//
// Workspace: [B * C * nvox] int64 accumulators, [B * C] maxima as bit patterns, [B * C] exponents k.
#include "push_accum.h"

namespace {

// max |x| of row blockIdx.y of [rows][len], as the bit pattern of |x|: non-negative floats order like unsigned integers,
// Inf lies above every finite value and every NaN above Inf, so one integer atomicMax per block keeps what the slice
// needs to know, in any order.  m starts at 0.
__global__ void __launch_bounds__(256) slice_absmax(const float* __restrict__ x, int64_t rows, int64_t len,
                                                    unsigned* __restrict__ m) {
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const float* p = x + r * len;
        unsigned u = 0;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x)
            u = max(u, __float_as_uint(p[i]) & 0x7fffffffu);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) u = max(u, (unsigned)__shfl_xor((int)u, o, 64));
        if ((threadIdx.x & 63) == 0 && u) atomicMax(m + r, u);
    }
}

// k = 62 - bits - e with m < 2^e (frexp: m = f * 2^e, 1/2 <= f < 1, denormals included); 0 for m = 0.  Dead: m NaN or Inf,
// and with G > 1 an m of 2^126 or more, where a contribution of up to G * m <= 3 m need not be a finite float.
__global__ void slice_exponent(const unsigned* __restrict__ m, int64_t rows, int bits, int G, int* __restrict__ k) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const unsigned u = m[r];
    int e = 0;
    if (u) (void)frexpf(__uint_as_float(u), &e);
    const bool dead = u >= 0x7f800000u || (G > 1 && e >= 127);
    k[r] = dead ? PUSH_FIXED_DEAD : (u ? 62 - bits - e : 0);
}

// out = (float)((double)acc * 2^-k): int64 -> double and double -> float both round to nearest even, the product is exact
__global__ void __launch_bounds__(256) fixed_finalize(const long long* __restrict__ acc, const int* __restrict__ k, int Bi,
                                                      int C, int64_t slices, int64_t nvox, float* __restrict__ out) {
    for (int64_t s = blockIdx.y; s < slices; s += gridDim.y) {
        const int ks = k[Bi == 1 ? s % C : s];
        const double inv = ks == PUSH_FIXED_DEAD ? 0.0 : __longlong_as_double((long long)(1023 - ks) << 52);
        const long long* a = acc + s * nvox;
        float* o = out + s * nvox;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x)
            o[i] = ks == PUSH_FIXED_DEAD ? __uint_as_float(0x7fc00000u) : (float)((double)a[i] * inv);
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// blocks along a slice and slices along y, about 2048 blocks in all
dim3 slice_grid(int64_t len, int64_t slices) {
    const int64_t gx = std::min<int64_t>(std::max<int64_t>(1, bfm_cdiv64(len, 1024)), 1024);
    const int64_t gy = std::min<int64_t>(slices, std::max<int64_t>(1, 2048 / gx));
    return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

extern "C" int bfm_grid_push_fixed_bits(int64_t P, const int* order, int D, int G) {
    if (P <= 0 || !order || D < 1 || D > 3 || G < 1 || G > 3) return BFM_E_ARG;
    int64_t T = 1;
    for (int a = 0; a < D; ++a) {
        if (order[a] < 0 || order[a] > 3) return BFM_E_ARG;
        T *= order[a] + 1;
    }
    if (P > (INT64_MAX / (T * G))) return BFM_E_ARG;
    const uint64_t n = (uint64_t)P * (uint64_t)T * (uint64_t)G;     // ceil(log2(n)): the bits of n - 1
    int bits = 0;
    while (bits < 64 && ((n - 1) >> bits) != 0) ++bits;
    return bits > PUSH_FIXED_MAX_BITS ? BFM_E_ARG : bits;
}

extern "C" size_t bfm_grid_push_fixed_workspace(int B, int C, int64_t nvox) {
    if (B <= 0 || C <= 0 || nvox <= 0) return 0;
    const size_t slices = (size_t)B * C;
    return align256(slices * (size_t)nvox * 8) + 2 * align256(slices * 4);
}

int push_fixed_begin(PushFixedPlan* plan, const float* inp, int Bi, int C, int64_t len, int B, int64_t nvox, int64_t P,
                     const int* order, int D, int G, void* ws, size_t ws_bytes, bfm_stream_t stream) {
    const int bits = bfm_grid_push_fixed_bits(P, order, D, G);
    if (bits < 0) return bits;
    if (!ws || ws_bytes < bfm_grid_push_fixed_workspace(B, C, nvox)) return BFM_E_ARG;
    const size_t slices = (size_t)B * C, acc_bytes = align256(slices * (size_t)nvox * 8), m_bytes = align256(slices * 4);
    char* base = static_cast<char*>(ws);
    unsigned* m = reinterpret_cast<unsigned*>(base + acc_bytes);
    int* k = reinterpret_cast<int*>(base + acc_bytes + m_bytes);
    if (hipMemsetAsync(base, 0, acc_bytes + m_bytes, bfm_s(stream)) != hipSuccess) return BFM_E_LAUNCH;
    const int64_t rows = (int64_t)Bi * C;
    hipLaunchKernelGGL(slice_absmax, slice_grid(len, rows), dim3(256), 0, bfm_s(stream), inp, rows, len, m);
    hipLaunchKernelGGL(slice_exponent, dim3((unsigned)bfm_cdiv64(rows, 256)), dim3(256), 0, bfm_s(stream), m, rows, bits, G,
                       k);
    *plan = PushFixedPlan{reinterpret_cast<unsigned long long*>(base), k, (int64_t)slices, nvox, Bi, C};
    return bfm_launch_status();
}

int push_fixed_end(const PushFixedPlan& plan, float* out, bfm_stream_t stream) {
    hipLaunchKernelGGL(fixed_finalize, slice_grid(plan.nvox, plan.slices_out), dim3(256), 0, bfm_s(stream),
                       reinterpret_cast<const long long*>(plan.acc), plan.k, plan.Bi, plan.C, plan.slices_out,
                       plan.nvox, out);
    return bfm_launch_status();
}
