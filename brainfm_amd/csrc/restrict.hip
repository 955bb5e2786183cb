// Separable spline operators along one axis: interpol.restrict (utils/interpol/restrict.py:9-122 -> grid_push on a
// meshgrid of three coordinate lists) and the backward of the separable cubic interpol.resize.
//
// A restrict / resize grid has one coordinate list per axis, so the (order + 1)^3-tap scatter or gather of nd.py factors
// into three axis passes.  Per axis the operator is a small sparse matrix: coordinate i of `coord[m]` touches node
// k = 0..order at bound_index(g0 + k) with spline_weight(order, g - g0 - k) * bound_sign(g0 + k) * mask_i -- axis_nodes
// and inbounds of spline_nodes.h, the device functions of the voxel-wise kernels, with the mask taken per axis against n
// (the 3-D inbounds mask of a separable grid is the product of the per-axis ones).
//
// The matrix is built on the device as a CSR table in either direction:
//   pull       row = coordinate i, order + 1 entries (k ascending), rowptr[i] = i * (order + 1);
//   transposed row = node j, its entries in ascending (i, k); entries whose value is exactly 0 (a node the `zero` bound
//              drops, a masked coordinate) are left out, as grid_push issues nothing for them.
// One deviation from axis_nodes, on request (ties_even): when all three orders of a call are 0 the reference leaves the
// generic path for iso0.py, whose node is round(g) -- a coordinate exactly halfway goes to the even node, where
// floor(g + 0.5) takes the upper one.  An integer factor under the 'f' / 'l' anchors puts every second sample there.
// One streaming pass applies a table along one axis of a [lead][X][Y][Z] block: out[.., r, ..] = sum_e val[e] *
// in[.., col[e], ..], e ascending within row r -- that entry order is the summation order, so the result is the same bit
// for bit from run to run.  Every output element is written (an empty row gives 0); nothing is added atomically.
//
// The passes are HBM-bound.  Along x and y the lanes run along z (coalesced, 16 bytes per lane where z is a multiple of
// 4).  Along z a block stages whole lines in an LDS tile with coalesced loads (odd pitch), computes from LDS and stores
// coalesced -- the form of prefilter_z_kernel; lines longer than the tile holds take the strided kernel.
#include "bfm_common.h"
#include "interp_bounds.h"
#include "spline_nodes.h"

namespace {

// pull direction; rowptr may be null (the staging table of the transposed build needs none)
__global__ void __launch_bounds__(256) axis_table_kernel(const float* __restrict__ coord, int m, int n, int order,
                                                         int bound, int extrap, int ties_even,
                                                         int32_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                         float* __restrict__ val) {
    const int T = order + 1;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += gridDim.x * blockDim.x) {
        if (rowptr) rowptr[i] = i * T;
        if (i == m) break;
        const float g = coord[i];
        const float mask = inbounds<1>(&g, &n, extrap);                       // this axis alone
        int idx[4];
        float w[4];
        axis_nodes<4>(g, order, n, bound, idx, w);
        if (ties_even && order == 0) {               // iso0.py:12: g.round(), a tie to the even node
            const int node = node_int(rintf(g));
            idx[0] = bound_index(node, n, bound);
            w[0] = (float)bound_sign(node, n, bound);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k <= order) {
                col[i * T + k] = idx[k];
                val[i * T + k] = w[k] * mask;
            }
    }
}

__device__ __forceinline__ bool entry_of_row(const int32_t* __restrict__ pcol, const float* __restrict__ pval, int e,
                                             int nent, int j) {
    return e < nent && pcol[e] == j && pval[e] != 0.f;
}

// transposed direction, step 1: one wave per node j counts the entries of the pull table that land on it
__global__ void __launch_bounds__(256) axis_table_count_kernel(const int32_t* __restrict__ pcol,
                                                               const float* __restrict__ pval, int nent, int n,
                                                               int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= n) return;
    int cnt = 0;
    for (int e0 = 0; e0 < nent; e0 += 64) cnt += __popcll(__ballot(entry_of_row(pcol, pval, e0 + lane, nent, j)));
    if (lane == 0) count[j] = cnt;
}

// step 2: the wave of node j sums the counts before it (its row start) and writes its entries in ascending (i, k)
__global__ void __launch_bounds__(256) axis_table_fill_kernel(const int32_t* __restrict__ pcol,
                                                              const float* __restrict__ pval, int nent, int n, int T,
                                                              const int32_t* __restrict__ count,
                                                              int32_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                              float* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= n) return;
    int before = 0;
    for (int r = lane; r < j; r += 64) before += count[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    int pos = before;
    for (int e0 = 0; e0 < nent; e0 += 64) {
        const int e = e0 + lane;
        const bool hit = entry_of_row(pcol, pval, e, nent, j);
        const unsigned long long b = __ballot(hit);
        if (hit) {
            const int p = pos + __popcll(b & ((1ull << lane) - 1ull));
            col[p] = e / T;
            val[p] = pval[e];
        }
        pos += __popcll(b);
    }
    if (lane == 0) {
        rowptr[j] = before;
        if (j == n - 1) rowptr[n] = pos;
    }
}

// [outer][n_in][inner] -> [outer][n_out][inner]; I: uint32_t when every index fits, int64_t otherwise.  V = float4 when
// inner is a multiple of 4 and both blocks start on 16 bytes (then `inner` and `total` count float4s), float otherwise.
__device__ __forceinline__ void fma_to(float& acc, float w, float v) { acc = fmaf(w, v, acc); }
__device__ __forceinline__ void fma_to(float4& acc, float w, const float4& v) {
    acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
}

template <typename I, typename V>
__global__ void __launch_bounds__(256) axis_pass_kernel(const V* __restrict__ in, I total, int n_in, I inner,
                                                        const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, const float* __restrict__ val,
                                                        int n_out, V* __restrict__ out) {
    for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
        const I q = i / inner, c = i - q * inner;
        const I l = q / (I)n_out;
        const int r = (int)(q - l * (I)n_out);
        const V* src = in + (int64_t)l * n_in * (int64_t)inner + (int64_t)c;
        const int e1 = rowptr[r + 1];
        V acc{};
        for (int e = rowptr[r]; e < e1; ++e) fma_to(acc, val[e], src[(int64_t)col[e] * (int64_t)inner]);
        out[i] = acc;
    }
}

// The contiguous axis: a block of 4 waves stages 4 * LPW whole lines in LDS (rows of n_in | 1 floats, coalesced loads).
// Lane j of a wave owns the output rows j, j + 64, ...: it reads each entry of a row once and applies it to the LPW
// lines of its wave, so the table is read once per LPW outputs, and the lanes of a wave store neighbouring outputs.
constexpr int LPW = 4;
__global__ void __launch_bounds__(256) axis_pass_z_kernel(const float* __restrict__ in, int64_t lines, int n_in,
                                                          const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col, const float* __restrict__ val,
                                                          int n_out, float* __restrict__ out) {
    extern __shared__ float tile[];                  // [4 * LPW][n_in | 1]
    constexpr int L = 4 * LPW;
    const int ld = n_in | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t l0 = (int64_t)blockIdx.x * L; l0 < lines; l0 += (int64_t)gridDim.x * L) {
        const int nl = (int)min<int64_t>(L, lines - l0);
        for (int line = wave; line < L; line += 4) {  // a line that does not exist is staged as zeros and never stored
            const float* src = in + (l0 + line) * n_in;
            for (int c = lane; c < n_in; c += 64) tile[line * ld + c] = line < nl ? src[c] : 0.f;
        }
        __syncthreads();
        const float* rows = tile + wave * LPW * ld;
        float* dst = out + (l0 + wave * LPW) * n_out;
        for (int r = lane; r < n_out; r += 64) {
            const int e1 = rowptr[r + 1];
            float acc[LPW];
#pragma unroll
            for (int k = 0; k < LPW; ++k) acc[k] = 0.f;
            for (int e = rowptr[r]; e < e1; ++e) {
                const int c = col[e];
                const float w = val[e];
#pragma unroll
                for (int k = 0; k < LPW; ++k) acc[k] = fmaf(w, rows[k * ld + c], acc[k]);
            }
#pragma unroll
            for (int k = 0; k < LPW; ++k)
                if (wave * LPW + k < nl) dst[(int64_t)k * n_out + r] = acc[k];
        }
        __syncthreads();
    }
}

constexpr int kMaxCoords = 1 << 24;                  // m * (order + 1) and the node indices stay far inside int32
constexpr int kTileBytes = 48 * 1024;              // 16 lines of up to 767 floats

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t bfm_spline_axis_table_workspace(int m, int n, int order) {
    if (m <= 0 || n <= 0 || order < 0 || order > 3 || m > kMaxCoords || n > kMaxCoords) return 0;
    const size_t nent = (size_t)m * (order + 1);
    return 2 * align256(nent * 4) + align256((size_t)n * 4);
}

extern "C" int bfm_spline_axis_table(const float* coord, int m, int n, int order, int bound, int extrapolate,
                                     int ties_even, int transpose, int32_t* rowptr, int32_t* col, float* val,
                                     void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (!coord || !rowptr || !col || !val || m <= 0 || n <= 0 || order < 0 || order > 3 || bound < 0 || bound > 6 ||
        extrapolate < 0 || extrapolate > 2 || ties_even < 0 || ties_even > 1 || transpose < 0 || transpose > 1)
        return BFM_E_ARG;
    if (m > kMaxCoords || n > kMaxCoords) return BFM_E_SHAPE;
    const int nblk = bfm_cdiv(m + 1, 256);
    if (!transpose) {
        hipLaunchKernelGGL(axis_table_kernel, dim3(nblk), dim3(256), 0, bfm_s(stream), coord, m, n, order, bound,
                           extrapolate, ties_even, rowptr, col, val);
        return bfm_launch_status();
    }
    if (!workspace || workspace_bytes < bfm_spline_axis_table_workspace(m, n, order)) return BFM_E_WORKSPACE;
    const int T = order + 1, nent = m * T;
    char* ws = static_cast<char*>(workspace);
    int32_t* pcol = reinterpret_cast<int32_t*>(ws);
    float* pval = reinterpret_cast<float*>(ws + align256((size_t)nent * 4));
    int32_t* count = reinterpret_cast<int32_t*>(ws + 2 * align256((size_t)nent * 4));
    hipLaunchKernelGGL(axis_table_kernel, dim3(nblk), dim3(256), 0, bfm_s(stream), coord, m, n, order, bound, extrapolate,
                       ties_even, (int32_t*)nullptr, pcol, pval);
    const int rblk = bfm_cdiv(n, 4);                 // 4 waves of 64 per block, one wave per node
    hipLaunchKernelGGL(axis_table_count_kernel, dim3(rblk), dim3(256), 0, bfm_s(stream), pcol, pval, nent, n, count);
    hipLaunchKernelGGL(axis_table_fill_kernel, dim3(rblk), dim3(256), 0, bfm_s(stream), pcol, pval, nent, n, T, count,
                       rowptr, col, val);
    return bfm_launch_status();
}

extern "C" int bfm_spline_axis_pass(const float* in, int64_t lead, int nx, int ny, int nz, int axis,
                                    const int32_t* rowptr, const int32_t* col, const float* val, int n_out, float* out,
                                    bfm_stream_t stream) {
    if (!in || !rowptr || !col || !val || !out || lead <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || axis < 0 || axis > 2 ||
        n_out <= 0)
        return BFM_E_ARG;
    const int d[3] = {nx, ny, nz};
    const int n_in = d[axis];
    int64_t outer = lead, inner = 1;
    for (int a = 0; a < axis; ++a) outer *= d[a];
    for (int a = axis + 1; a < 3; ++a) inner *= d[a];
    const int64_t limit = (int64_t)1 << 46;          // elements of either block: far beyond any memory, far inside int64
    if (outer > limit / n_in / inner || outer > limit / n_out / inner) return BFM_E_SHAPE;
    const int64_t total = outer * n_out * inner;
    const size_t tile_bytes = (size_t)4 * LPW * (n_in | 1) * sizeof(float);
    if (axis == 2 && tile_bytes <= (size_t)kTileBytes) {
        const int nb = (int)std::min<int64_t>(16384, bfm_cdiv64(outer, 4 * LPW));
        hipLaunchKernelGGL(axis_pass_z_kernel, dim3(nb), dim3(256), tile_bytes, bfm_s(stream), in, outer, n_in, rowptr, col,
                           val, n_out, out);
        return bfm_launch_status();
    }
    const bool vec = inner % 4 == 0 && (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const int64_t per = vec ? 4 : 1;
    const int nb = (int)std::min<int64_t>(16384, bfm_cdiv64(total / per, 256));
    const bool small = total < ((int64_t)1 << 31) && outer * n_in * inner < ((int64_t)1 << 31);
#define BFM_AXIS_PASS(I, V)                                                                                            \
    hipLaunchKernelGGL((axis_pass_kernel<I, V>), dim3(nb), dim3(256), 0, bfm_s(stream), reinterpret_cast<const V*>(in),  \
                       (I)(total / per), n_in, (I)(inner / per), rowptr, col, val, n_out, reinterpret_cast<V*>(out))
    if (small && vec) BFM_AXIS_PASS(uint32_t, float4);
    else if (small) BFM_AXIS_PASS(uint32_t, float);
    else if (vec) BFM_AXIS_PASS(int64_t, float4);
    else BFM_AXIS_PASS(int64_t, float);
#undef BFM_AXIS_PASS
    return bfm_launch_status();
}
