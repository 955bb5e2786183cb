// Per-axis spline nodes of the interpol grid kernels (utils/interpol/nd.py:44-75 and :368-391, splines.py:30-43, :90-103
// and :149-157), shared by the voxel-wise kernels of spline_grid.hip, grid_hess.hip and label_pull.hip (through
// grid_kernels.h) and the separable axis tables of restrict.hip: the weight and its first and second derivative, node k
// of one axis (index, weight * sign, derivatives * sign) in one definition, and the inbounds mask (extrapolate 0 no /
// 1 yes / 2 hist).
#pragma once
#include "bfm_common.h"
#include "interp_bounds.h"

// splines.py:30-43
__device__ __forceinline__ float spline_weight(int order, float x) {
    if (order == 0) return 1.f;
    x = fabsf(x);
    if (order == 1) return 1.f - x;
    if (order == 2) {
        const float t = 1.5f - x;
        return x < 0.5f ? 0.75f - x * x : 0.5f * (t * t);
    }
    const float t = 2.f - x;
    return x < 1.f ? (x * x * (x - 2.f) * 3.f + 4.f) / 6.f : (t * t * t) / 6.f;
}

// splines.py:90-103: _fastgrad(|x|) * sign(x), sign(0) = 0
__device__ __forceinline__ float spline_dweight(int order, float x) {
    if (order == 0) return 0.f;
    const float s = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
    x = fabsf(x);
    float g;
    if (order == 1) g = 1.f;
    else if (order == 2) g = x < 0.5f ? -2.f * x : x - 1.5f;
    else {
        const float t = 2.f - x;
        g = x < 1.f ? x * (x * 1.5f - 2.f) : -0.5f * (t * t);
    }
    return g * s;
}

// splines.py:149-157: fasthess, even in x (no sign factor); 0 for orders 0 and 1
__device__ __forceinline__ float spline_d2weight(int order, float x) {
    if (order < 2) return 0.f;
    x = fabsf(x);
    if (order == 2) return x < 0.5f ? -2.f : 1.f;
    return x < 1.f ? 3.f * x - 2.f : 2.f - x;
}

// coordinates beyond +-2^30 voxels have no meaning; the clamp keeps grid0 + k inside what bound_index maps to [0, n-1]
__device__ __forceinline__ int node_int(float f) { return (int)fminf(fmaxf(f, -1073741824.f), 1073741824.f); }

// Node k of one axis (nd.py:44-75 and :368-391), the one definition every kernel of the family takes its nodes from: the
// label pull's tie rule and every bit-for-bit comparison between kernels rest on that.  idx = bound_index(grid0 + k),
// w = weight * sign, and with D >= 1 *dw = fastgrad * sign, with D == 2 *d2w = fasthess * sign; a derivative that D does
// not ask for is not written and its pointer may be left out.  ISO1 (order 1 only): the slope of iso1.py (-1 at the
// lower node, +1 at the upper), not the sign(x) of the generic path's fastgrad.  k > order: a padded tap, weight 0 and
// the index of tap 0.  k may be a run-time value: the kernels that walk the footprint slab by slab in a rolled loop call
// this directly, since an array of nodes read at a run-time index would go to scratch.
template <int D = 0, bool ISO1 = false>
__device__ __forceinline__ void axis_node(float g, int order, int n, int b, int k, int& idx, float& w, float* dw = nullptr,
                                          float* d2w = nullptr) {
    const float g0f = floorf(g - 0.5f * (float)(order - 1));
    const float dist0 = g - g0f;
    const int g0 = node_int(g0f);
    const bool used = k <= order;
    const int node = used ? g0 + k : g0;
    const float s = used ? (float)bound_sign(node, n, b) : 0.f;
    idx = bound_index(node, n, b);
    const float d = dist0 - (float)k;
    w = spline_weight(order, d) * s;
    if (D >= 1) *dw = (ISO1 ? (k == 0 ? -1.f : 1.f) : spline_dweight(order, d)) * s;
    if (D >= 2) *d2w = spline_d2weight(order, d) * s;
}

// the T nodes of one axis in registers
template <int T, int D = 0, bool ISO1 = false>
__device__ __forceinline__ void axis_nodes(float g, int order, int n, int b, int (&idx)[T], float (&w)[T],
                                           float* dw = nullptr, float* d2w = nullptr) {
#pragma unroll
    for (int k = 0; k < T; ++k)
        axis_node<D, ISO1>(g, order, n, b, k, idx[k], w[k], D >= 1 ? dw + k : nullptr, D >= 2 ? d2w + k : nullptr);
}

// the inbounds mask of a coordinate g[0..D) against the extents n[0..D): 1 inside, 0 outside
template <int D>
__device__ __forceinline__ float inbounds(const float* g, const int* n, int extrap) {
    if (extrap == 0 || extrap == 2) {
        const float thr = extrap == 2 ? 0.5f + 5e-2f : 5e-2f;
        bool in = true;
#pragma unroll
        for (int a = 0; a < D; ++a) in = in && (g[a] > -thr) && (g[a] < (float)(n[a] - 1) + thr);
        return in ? 1.f : 0.f;
    }
    return 1.f;
}
