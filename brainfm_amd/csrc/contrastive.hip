// Contrastive feature loss of the head-less pre-training mode: loss_feat_contrastive of
// Trainer/models/criterion.py:96-109 on the feature maps ContrastiveProcessor (Trainer/models/joiner.py:136-147) leaves,
// with its gradient w.r.t. the RAW decoder outputs of both samples, in one pass over the two channels-last maps.
//
//   x -> p : F.normalize(dim=1) n_norm times (unit_feat of the backbone + the processor = 2), eps 1e-12; the same for y -> q
//   S   = sum_j p_j
//   num = sum_c exp(p_c q_c / alpha)
//   den = sum_i [ exp(p_i^2 / beta) + exp((p_i S - p_i^2) / gamma) ]          (the reference's loop over i, written O(C))
//   loss = mean_v log(den) - log(num)
//   d loss_v / d p_k = [2 a_k p_k / beta + (b_k (S - 2 p_k) + T) / gamma] / den - w_k q_k / alpha
//   d loss_v / d q_k = - w_k p_k / alpha
//     a_i = exp(p_i^2 / beta), b_i = exp((p_i S - p_i^2) / gamma), T = sum_i b_i p_i, w_c = exp(p_c q_c / alpha) / num
//   and back through each normalisation as bfm_normalize_bwd does: |x| > eps: (g - x^ <g, x^>) / |x|, else g / eps.
//
// Every exponent has the voxel's largest one subtracted first (one maximum for den, one for num), so fp32 stays finite
// where the reference's fp32 overflows (exponents up to sqrt(C-1) / (2 gamma) and 1 / alpha); where the reference is finite
// the value is the same.
//
// Work split.  A voxel belongs to a group of LPV adjacent lanes, each holding NCH channels in registers; sums and maxima
// over the channels are xor-shuffles inside the group, so nothing goes through LDS but the block's loss partial.
//   C == 64 (the shipped width): LPV = 8, NCH = 8 -- 8 voxels per wave; lane j holds channels 4j..4j+3 and 32+4j..32+4j+3,
//     so each of the two 16-byte loads (and stores) of a group covers 128 contiguous bytes.  The ~14 reductions of a voxel
//     cost 3 shuffle steps for 8 voxels at once; with lane = channel (one voxel per wave) they cost 6 steps per voxel, 16
//     times the cross-lane work, and that form is bound by the shuffles instead of by HBM.
//   any other 2 <= C <= 64: one wave per voxel, lane = channel (lanes >= C masked).  Correct for every width; not tuned.
// The loss is summed in fp64: per lane over its voxels, a fixed tree per block, the block partials folded in order by a
// second launch -- no atomics, the same bits on every run.
#include "bfm_common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;

template <int LPV>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LPV / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int LPV>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = LPV / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double block_sum(double v, double* red) {          // NT threads, fixed tree
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(NT) fold_kernel(const double* __restrict__ part, int nb, double scale,
                                                  double* __restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += NT) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s * scale;
}

// Channel of register k of lane `sub`: float4 pieces laid side by side across the group (NCH % 4 == 0), or lane = channel.
template <int NCH, int LPV>
__device__ __forceinline__ int chan_of(int sub, int k) {
    return NCH % 4 == 0 ? (k / 4) * (4 * LPV) + sub * 4 + (k % 4) : sub * NCH + k;
}

template <int NCH, int LPV>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int sub, int C, bool ok, float (&x)[NCH]) {
    if constexpr (NCH % 4 == 0) {
#pragma unroll
        for (int k = 0; k < NCH; k += 4) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) t = *reinterpret_cast<const float4*>(row + chan_of<NCH, LPV>(sub, k));
            x[k] = t.x; x[k + 1] = t.y; x[k + 2] = t.z; x[k + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = chan_of<NCH, LPV>(sub, k);
            x[k] = (ok && c < C) ? row[c] : 0.f;
        }
    }
}

template <int NCH, int LPV>
__device__ __forceinline__ void store_row(float* __restrict__ row, int sub, int C, bool ok, const float (&x)[NCH]) {
    if constexpr (NCH % 4 == 0) {
#pragma unroll
        for (int k = 0; k < NCH; k += 4)
            if (ok) *reinterpret_cast<float4*>(row + chan_of<NCH, LPV>(sub, k)) = make_float4(x[k], x[k + 1], x[k + 2], x[k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = chan_of<NCH, LPV>(sub, k);
            if (ok && c < C) row[c] = x[k];
        }
    }
}

// x -> x / max(|x|, eps); returns |x|
template <int NCH, int LPV>
__device__ __forceinline__ float normalize(const float (&x)[NCH], float eps, float (&y)[NCH]) {
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) ss += x[k] * x[k];
    const float nrm = sqrtf(group_sum<LPV>(ss));
    const float inv = 1.f / fmaxf(nrm, eps);
#pragma unroll
    for (int k = 0; k < NCH; ++k) y[k] = x[k] * inv;
    return nrm;
}

// gradient w.r.t. the normalised y = x / max(|x|, eps) -> gradient w.r.t. x (bfm_normalize_bwd's two branches)
template <int NCH, int LPV>
__device__ __forceinline__ void normalize_bwd(const float (&y)[NCH], float nrm, float eps, float (&g)[NCH]) {
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) dot += g[k] * y[k];
    dot = group_sum<LPV>(dot);                               // outside the branch: the shuffles stay convergent
    const bool big = nrm > eps;
    const float sc = 1.f / (big ? nrm : eps);
#pragma unroll
    for (int k = 0; k < NCH; ++k) g[k] = (big ? g[k] - y[k] * dot : g[k]) * sc;
}

// MASKED: lanes whose channel is >= C hold zeros and are kept out of the maxima and sums (the lane = channel form).
template <int NCH, int LPV, bool MASKED>
__global__ void __launch_bounds__(NT) contrastive_kernel(const float* __restrict__ X, const float* __restrict__ Y, int C,
                                                         int64_t nvox, int n_norm, float eps, float inv_a, float inv_b,
                                                         float inv_g, float gscale, float* __restrict__ dX,
                                                         float* __restrict__ dY, float* __restrict__ Pn,
                                                         float* __restrict__ Qn, double* __restrict__ part) {
    __shared__ double red[NT];
    constexpr int VPB = NT / LPV;                            // voxels per block and trip
    const int sub = threadIdx.x % LPV, slot = threadIdx.x / LPV;
    const int64_t trips = bfm_cdiv64(nvox, VPB);
    bool live[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) live[k] = !MASKED || chan_of<NCH, LPV>(sub, k) < C;
    double acc = 0.0;
    for (int64_t it = blockIdx.x; it < trips; it += gridDim.x) {      // the same trip count for the whole block
        const int64_t v = it * VPB + slot;
        const bool ok = v < nvox;
        const int64_t base = v * C;
        float p[3][NCH], q[3][NCH];                          // [j]: after j normalisations (stage n_norm.. 2: copies)
        float np[2], nq[2];
        load_row<NCH, LPV>(X + base, sub, C, ok, p[0]);
        load_row<NCH, LPV>(Y + base, sub, C, ok, q[0]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j < n_norm) {
                np[j] = normalize<NCH, LPV>(p[j], eps, p[j + 1]);
                nq[j] = normalize<NCH, LPV>(q[j], eps, q[j + 1]);
            } else {
                np[j] = nq[j] = 1.f;
#pragma unroll
                for (int k = 0; k < NCH; ++k) { p[j + 1][k] = p[j][k]; q[j + 1][k] = q[j][k]; }
            }
        }
        const float (&pp)[NCH] = p[2];
        const float (&qq)[NCH] = q[2];
        if (Pn) store_row<NCH, LPV>(Pn + base, sub, C, ok, pp);
        if (Qn) store_row<NCH, LPV>(Qn + base, sub, C, ok, qq);

        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) s += pp[k];
        const float S = group_sum<LPV>(s);
        float e1[NCH], e2[NCH], en[NCH];
        float m = -INFINITY, mn = -INFINITY;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const float sq = pp[k] * pp[k];
            e1[k] = sq * inv_b;
            e2[k] = (pp[k] * S - sq) * inv_g;
            en[k] = pp[k] * qq[k] * inv_a;
            if (live[k]) {
                m = fmaxf(m, fmaxf(e1[k], e2[k]));
                mn = fmaxf(mn, en[k]);
            }
        }
        m = group_max<LPV>(m);
        mn = group_max<LPV>(mn);
        float den = 0.f, T = 0.f, num = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            // a_k, b_k, exp(p_k q_k / alpha), all over their maximum.  The arguments are <= 0, so the hardware exponential's
            // error, |x| 2^-24 relative, is at most 0.37 * 2^-24 of the largest term: below an fp32 rounding of the sums
            e1[k] = live[k] ? __expf(e1[k] - m) : 0.f;
            e2[k] = live[k] ? __expf(e2[k] - m) : 0.f;
            en[k] = live[k] ? __expf(en[k] - mn) : 0.f;
            den += e1[k] + e2[k];
            T += e2[k] * pp[k];
            num += en[k];
        }
        den = group_sum<LPV>(den);
        T = group_sum<LPV>(T);
        num = group_sum<LPV>(num);
        if (ok && sub == 0) acc += ((double)m - (double)mn) + ((double)logf(den) - (double)logf(num));
        if (!dX) continue;                                   // the value only (uniform over the grid)

        const float rden = 1.f / den, rnum = 1.f / num;
        float gp[NCH], gq[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const float w = en[k] * rnum;
            const float dden = 2.f * e1[k] * pp[k] * inv_b + (e2[k] * (S - 2.f * pp[k]) + T) * inv_g;
            gp[k] = live[k] ? gscale * (dden * rden - w * qq[k] * inv_a) : 0.f;
            gq[k] = gscale * (-(w * pp[k]) * inv_a);
        }
#pragma unroll
        for (int j = 1; j >= 0; --j) {
            if (j < n_norm) {
                normalize_bwd<NCH, LPV>(p[j + 1], np[j], eps, gp);
                normalize_bwd<NCH, LPV>(q[j + 1], nq[j], eps, gq);
            }
        }
        store_row<NCH, LPV>(dX + base, sub, C, ok, gp);
        store_row<NCH, LPV>(dY + base, sub, C, ok, gq);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

}  // namespace

extern "C" size_t bfm_loss_contrastive_workspace(void) { return (size_t)MAX_BLOCKS * sizeof(double); }

extern "C" int bfm_loss_contrastive(const float* featP, const float* featQ, int C, int64_t nvox, int n_norm, float eps,
                                    float alpha, float beta, float gamma, float coef, float* dP, float* dQ, float* p_out,
                                    float* q_out, double* loss_out, void* workspace, size_t workspace_bytes,
                                    bfm_stream_t stream) {
    if (!featP || !featQ || !loss_out || !workspace || (dP == nullptr) != (dQ == nullptr) || nvox <= 0 || n_norm < 0 ||
        n_norm > 2 || !(eps > 0.f) || !(alpha > 0.f) || !(beta > 0.f) || !(gamma > 0.f) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
        return BFM_E_ARG;
    if (C < 2 || C > 64) return BFM_E_SHAPE;
    if (workspace_bytes < bfm_loss_contrastive_workspace()) return BFM_E_WORKSPACE;
    const uintptr_t any = reinterpret_cast<uintptr_t>(featP) | reinterpret_cast<uintptr_t>(featQ) |
                          reinterpret_cast<uintptr_t>(dP) | reinterpret_cast<uintptr_t>(dQ) |
                          reinterpret_cast<uintptr_t>(p_out) | reinterpret_cast<uintptr_t>(q_out);
    double* part = static_cast<double*>(workspace);
    const bool wide = C == 64 && (any & 15) == 0;            // 16-byte accesses need 16-byte aligned maps
    const int nb = (int)std::min<int64_t>(MAX_BLOCKS, bfm_cdiv64(nvox, wide ? NT / 8 : NT / 64));
    const float gscale = (float)((double)coef / (double)nvox);
    const float ia = 1.f / alpha, ib = 1.f / beta, ig = 1.f / gamma;
    if (wide)
        hipLaunchKernelGGL((contrastive_kernel<8, 8, false>), dim3(nb), dim3(NT), 0, bfm_s(stream), featP, featQ, C, nvox,
                           n_norm, eps, ia, ib, ig, gscale, dP, dQ, p_out, q_out, part);
    else
        hipLaunchKernelGGL((contrastive_kernel<1, 64, true>), dim3(nb), dim3(NT), 0, bfm_s(stream), featP, featQ, C, nvox,
                           n_norm, eps, ia, ib, ig, gscale, dP, dQ, p_out, q_out, part);
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(NT), 0, bfm_s(stream), part, nb, 1.0 / (double)nvox, loss_out);
    return bfm_launch_status();
}
