// Boundary rules of the interpol grid kernels (utils/interpol/bounds.py:24-89), shared by the linear and
// the spline kernels of spline_grid.hip, grid_hess.hip and label_pull.hip: where an out-of-range node index lands (bound_index) and
// the sign its value takes (bound_sign).  b: 0 zero, 1 replicate, 2 dct1, 3 dct2, 4 dst1, 5 dst2, 6 dft (bounds.py:8-15).
// For every b in 0..6 and |i| <= 2^30, bound_index returns an index in [0, n-1].
#pragma once
#include "bfm_common.h"

// ---- interpol bounds (utils/interpol/bounds.py:24-89)
__device__ __forceinline__ int imod(int a, int m) { int r = a % m; return r < 0 ? r + m : r; }

__device__ __forceinline__ int bound_index(int i, int n, int b) {
    switch (b) {
        case 0: case 1: return min(max(i, 0), n - 1);
        case 3: case 5: {
            const int n2 = n * 2;
            i = i < 0 ? n2 - 1 - imod(-i - 1, n2) : imod(i, n2);
            return i >= n ? n2 - 1 - i : i;
        }
        case 2: {
            if (n == 1) return 0;
            const int n2 = (n - 1) * 2;
            i = imod(abs(i), n2);
            return i >= n ? n2 - i : i;
        }
        case 4: {
            const int n2 = 2 * (n + 1);
            i = i < 0 ? -i - 2 : i;
            i = imod(i, n2);
            i = i > n ? n2 - 2 - i : i;
            i = i == -1 ? 0 : i;
            return i == n ? n - 1 : i;
        }
        case 6: return imod(i, n);
        default: return i;
    }
}

__device__ __forceinline__ int bound_sign(int i, int n, int b) {
    switch (b) {
        case 4: {
            if (n == 1) return 1;
            const int n2 = 2 * (n + 1);
            i = i < 0 ? n - 1 - i : i;
            i = imod(i, n2);
            int x = i == 0 ? 0 : 1;
            x = (imod(i, n + 1) == n) ? 0 : x;
            i = i / (n + 1);
            return (i & 1) ? -x : x;
        }
        case 5: {
            i = i < 0 ? n - 1 - i : i;
            i = i / n;
            return (i & 1) ? -1 : 1;
        }
        case 0: return (i < 0 || i >= n) ? 0 : 1;
        default: return 1;
    }
}
