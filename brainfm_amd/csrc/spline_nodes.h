// Per-axis spline nodes of the interpol grid kernels (utils/interpol/nd.py:44-75, splines.py:30-43 and :90-103), shared by
// the voxel-wise kernels of spline_grid.hip and grid_hess.hip and the separable axis tables of restrict.hip: the weight and
// its first and second derivative (splines.py:149-157), the nodes of one axis (index, weight * sign, derivative * sign) and
// the inbounds mask (extrapolate 0 no / 1 yes / 2 hist).
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

// nodes of one axis (nd.py:44-75): off[k] = bound_index * stride, w[k] = weight * sign, dw[k] = fastgrad * sign
template <int T, bool GRAD>
__device__ __forceinline__ void axis_nodes(float g, int order, int n, int b, int (&idx)[T], float (&w)[T], float (&dw)[T]) {
    const float g0f = floorf(g - 0.5f * (float)(order - 1));
    const float dist0 = g - g0f;
    // coordinates beyond +-2^30 voxels have no meaning; the clamp keeps grid0 + k inside what bound_index maps to [0, n-1]
    const int g0 = (int)fminf(fmaxf(g0f, -1073741824.f), 1073741824.f);
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const bool used = k <= order;
        const int node = used ? g0 + k : g0;
        const float s = used ? (float)bound_sign(node, n, b) : 0.f;
        idx[k] = bound_index(node, n, b);
        const float d = dist0 - (float)k;
        w[k] = spline_weight(order, d) * s;
        dw[k] = GRAD ? spline_dweight(order, d) * s : 0.f;
    }
}

// splines.py:149-157: fasthess, even in x (no sign factor); 0 for orders 0 and 1
__device__ __forceinline__ float spline_d2weight(int order, float x) {
    if (order < 2) return 0.f;
    x = fabsf(x);
    if (order == 2) return x < 0.5f ? -2.f : 1.f;
    return x < 1.f ? 3.f * x - 2.f : 2.f - x;
}

// axis_nodes with the second derivative as well (nd.py:368-391): d2w[k] = fasthess * sign.  ISO1 (order 1 only, T = 2):
// the slope of iso1.py (-1 at the lower node, +1 at the upper), not the sign(x) of the generic path's fastgrad.  A sibling
// of axis_nodes, whose instantiations stay as they are.
template <int T, bool ISO1>
__device__ __forceinline__ void axis_nodes2(float g, int order, int n, int b, int (&idx)[T], float (&w)[T], float (&dw)[T],
                                            float (&d2w)[T]) {
    const float g0f = floorf(g - 0.5f * (float)(order - 1));
    const float dist0 = g - g0f;
    const int g0 = (int)fminf(fmaxf(g0f, -1073741824.f), 1073741824.f);
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const bool used = k <= order;
        const int node = used ? g0 + k : g0;
        const float s = used ? (float)bound_sign(node, n, b) : 0.f;
        idx[k] = bound_index(node, n, b);
        const float d = dist0 - (float)k;
        w[k] = spline_weight(order, d) * s;
        dw[k] = (ISO1 ? (k == 0 ? -1.f : 1.f) : spline_dweight(order, d)) * s;
        d2w[k] = spline_d2weight(order, d) * s;
    }
}

__device__ __forceinline__ float inbounds(float gx, float gy, float gz, int nx, int ny, int nz, int extrap) {
    if (extrap == 0 || extrap == 2) {
        const float thr = extrap == 2 ? 0.5f + 5e-2f : 5e-2f;
        const bool in = (gx > -thr) && (gx < (float)(nx - 1) + thr) && (gy > -thr) && (gy < (float)(ny - 1) + thr) &&
                        (gz > -thr) && (gz < (float)(nz - 1) + thr);
        return in ? 1.f : 0.f;
    }
    return 1.f;
}
