// How the scatter kernels of the interpol grid family (spline_push, padded_push3d, linear_push3d of spline_grid.hip and
// spline_pushgrad3d of grid_hess.hip) add a contribution to its node: one policy type, the kernels' last template
// parameter.
//
//   AccumFloat  one global_atomic_add_f32 per contribution into the zeroed fp32 output: the summation order, and so the
//               last bit, is not reproducible.  The default ("atomic") route.
//   AccumFixed  the contribution c of output slice (b, ch), the same fp32 value the float route adds, becomes the integer
//               q = rint(c * 2^k) (round to nearest even; the product is exact in double) and goes into an int64
//               accumulator with one global_atomic_add_x2.  Integer addition is associative, so the sum does not depend
//               on the arrival order, the lane mapping or the launch shape.  k = 62 - bits - e per slice, where the slice of
//               the input has max |x| = m < 2^e and bits = ceil(log2(P * T * G)) for P points per batch item, T taps per
//               point and |c| <= G * m (push_fixed.hip); so |sum q| <= P * T * (G * 2^(62 - bits) + 1/2) < 2^63 whatever
//               the input holds.  A slice whose m is NaN or Inf takes no part (k = PUSH_FIXED_DEAD) and is written as NaN
//               by the finalize pass; a slice of zeros has k = 0 and integer zeros to add.
//
// A kernel's last two arguments are `typename ACC::Cell* __restrict__ out`, [B][C][vol] cells that are zero on entry, and
// `typename ACC::Aux aux`.  Its pointer arithmetic is what it was on float*; once per channel it asks the policy for
// the Scale of the slice, skips a dead one, and hands every contribution to ACC::add.  For AccumFloat Aux and Scale are
// empty and dead() is constant, which leaves the kernels' instructions as they were before the policies.
#pragma once
#include <limits.h>

#include "bfm_common.h"

constexpr int PUSH_FIXED_DEAD = INT_MIN;      // k of a slice whose maximum is NaN or Inf
constexpr int PUSH_FIXED_MAX_BITS = 40;       // bits beyond this are refused (bfm_grid_push_fixed_bits)

struct AccumFloat {
    using Cell = float;
    struct Aux {};
    struct Scale {};
    // sin: the slice of the input, batch 0 for a broadcast input
    __device__ __forceinline__ static Scale scale(Aux, int64_t sin) { return {}; }
    __device__ __forceinline__ static constexpr bool dead(Scale) { return false; }
    __device__ __forceinline__ static void add(float* p, float c, Scale) { atomicAdd(p, c); }
};

struct AccumFixed {
    using Cell = unsigned long long;          // int64 two's complement
    using Aux = const int*;                   // [Bi][C]: k of every slice of the input
    using Scale = double;                     // 2^k, 0 for a dead slice
    __device__ __forceinline__ static Scale scale(Aux k, int64_t sin) {
        const int ks = k[sin];
        // 2^k from its exponent field: 62 - 40 - 128 <= k <= 62 + 149, well inside the normal doubles
        return ks == PUSH_FIXED_DEAD ? 0.0 : __longlong_as_double((long long)(ks + 1023) << 52);
    }
    __device__ __forceinline__ static bool dead(Scale s) { return s == 0.0; }
    __device__ __forceinline__ static void add(unsigned long long* p, float c, Scale s) {
        atomicAdd(p, (unsigned long long)(long long)rint((double)c * s));
    }
};

// The three light passes around a fixed-point push (push_fixed.hip).  `ws` is the caller's workspace of at least
// bfm_grid_push_fixed_workspace(B, C, nvox) bytes.
struct PushFixedPlan { unsigned long long* acc; const int* k; int64_t slices_out, nvox; int Bi, C; };

// Zeroes the accumulators, takes max |x| of each of the Bi * C slices of `inp` (len floats each) on the device and turns
// it into the slice's k.  P, order[0..D) and G as in bfm_grid_push_fixed_bits.
int push_fixed_begin(PushFixedPlan* plan, const float* inp, int Bi, int C, int64_t len, int B, int64_t nvox, int64_t P,
                     const int* order, int D, int G, void* ws, size_t ws_bytes, bfm_stream_t stream);
// out[b][c][v] = (float)((double)acc * 2^-k), NaN for a dead slice; every element of out is written
int push_fixed_end(const PushFixedPlan& plan, float* out, bfm_stream_t stream);
