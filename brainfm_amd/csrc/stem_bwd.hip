// Backward of the first SingleConv of a conditioned network (GroupNorm(1, Cin) + Conv3d(Cin, Cout, 3), Cin in {2,3,4},
// Trainer/models/__init__.py:423-437 with backbone.py:21-26 num_cond; buildingblocks.py:31-60) in ONE correlation.
// The layer's input is data, so no input gradient is wanted; what is wanted is dW and the 2 Cin numbers dgamma, dbeta.
// With xn[u,c] = scale_c x[u,c] + shift_c inside the volume (0 outside), scale_c = gamma_c rstd,
// shift_c = beta_c - mean rstd gamma_c, and over the RAW input
//
//     Q[o,c,t] = sum over v with v+t inside of dP[v,o] x[v+t,c]        S[o,t] = sum over v with v+t inside of dP[v,o]
//
// (S is Q of an extra channel that is 1 inside the volume), exactly
//
//     dW[o,c,t] = scale_c Q[o,c,t] + shift_c S[o,t]
//     dgamma_c  = rstd sum_{o,t} W[o,c,t] (Q[o,c,t] - mean S[o,t])
//     dbeta_c   =      sum_{o,t} W[o,c,t] S[o,t]
//
// so the whole backward is one weight-gradient GEMM, M = Cout, N = 27 (Cin + 1) <= 135, K = voxels, on the exact-fp32
// matrix core (v_mfma_f32_32x32x2_f32), and a fold of Cout x N numbers.  No data-gradient convolution, no dXn, no gn_bwd.
//
// stem_mc_bwd_kernel<COUT>: persistent workgroups over 4x4x16-voxel tiles.  Per tile the dP tile [256][COUT] and the
// (Cin+1)-plane input tile with its one-voxel halo [Cin+1][6*6*18] (zero outside the volume, the indicator plane too:
// zero padding and S fall out of the same loads) are staged in LDS, so dP is read from HBM once.  Wave w owns the 32
// columns (c', tap) = 32 w .. 32 w + 31 of all COUT rows; a K step is two x-neighbouring voxels.  Accumulators stay in
// registers over a workgroup's tiles; one fp32 partial per workgroup, folded in fp64 in split order (no atomics: the
// same bits on every run).
#include "bfm_common.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int ST_Z = 4, ST_Y = 4, ST_X = 16;
constexpr int SH_Y = ST_Y + 2, SH_X = ST_X + 2;
constexpr int ST_VOX = ST_Z * ST_Y * ST_X;                  // 256
constexpr int SH_VOX = (ST_Z + 2) * SH_Y * SH_X;            // 648
constexpr int SH_PLANE = SH_VOX + 5;                        // odd pitch: the planes start on different banks
constexpr int SB_MAX_SPLITS = 512;
constexpr int SB_GROUPS = 16;                               // second level of the fold

struct StemBwdParams {
    const float* dP;                  // [D][H][W][COUT]
    const float* x;                   // [D][H][W][Cin]
    int Cin, D, H, W;
    int nby, nbx, ntiles;
    float* part;                      // [S][COUT][27 (Cin+1)]
};

static inline int sb_lds_bytes(int Cin, int Cout) { return (ST_VOX * Cout + (Cin + 1) * SH_PLANE) * (int)sizeof(float); }

template <int COUT>
__global__ void __launch_bounds__(320) stem_mc_bwd_kernel(const StemBwdParams p) {
    extern __shared__ float sb_lds[];
    constexpr int MB = COUT / 32;
    float* dPs = sb_lds;                                    // [256][COUT]
    float* Xs = sb_lds + ST_VOX * COUT;                     // [Cin+1][SH_PLANE]
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63, l32 = lane & 31, lh = lane >> 5;
    const int CP = p.Cin + 1, ncol = 27 * CP;
    const int col = wave * 32 + l32;
    const bool col_ok = col < ncol;
    const int cc = col_ok ? col / 27 : 0;
    const int tap = col_ok ? col - cc * 27 : 0;
    const int boff = cc * SH_PLANE + ((tap / 9) * SH_Y + (tap / 3) % 3) * SH_X + tap % 3 + lh;
    floatx16 acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;

    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int bx = tile % p.nbx;
        const int t2 = tile / p.nbx;
        const int by = t2 % p.nby, bz = t2 / p.nby;
        const int z0 = bz * ST_Z, y0 = by * ST_Y, x0 = bx * ST_X;
        __syncthreads();                                    // the previous tile's reads are done
        for (int i = tid; i < ST_VOX * (COUT / 4); i += nthr) {
            const int v = i / (COUT / 4), c4 = i - v * (COUT / 4);
            const int z = z0 + (v >> 6), y = y0 + ((v >> 4) & 3), x = x0 + (v & 15);
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (z < p.D && y < p.H && x < p.W)
                val = *reinterpret_cast<const float4*>(p.dP + ((int64_t)(z * p.H + y) * p.W + x) * COUT + c4 * 4);
            *reinterpret_cast<float4*>(dPs + v * COUT + c4 * 4) = val;
        }
        for (int i = tid; i < SH_VOX * CP; i += nthr) {
            const int hv = i / CP, c = i - hv * CP;
            const int hz = hv / (SH_Y * SH_X);
            const int r = hv - hz * (SH_Y * SH_X);
            const int hy = r / SH_X, hx = r - hy * SH_X;
            const int zz = z0 + hz - 1, yy = y0 + hy - 1, xx = x0 + hx - 1;
            float val = 0.f;
            if (zz >= 0 && zz < p.D && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W)
                val = c < p.Cin ? p.x[((int64_t)(zz * p.H + yy) * p.W + xx) * p.Cin + c] : 1.f;
            Xs[c * SH_PLANE + hv] = val;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < ST_Z * ST_Y; ++r) {
            const int zl = r >> 2, yl = r & 3;
            const float* arow = dPs + (r * ST_X + lh) * COUT + l32;
            const float* brow = Xs + boff + (zl * SH_Y + yl) * SH_X;
#pragma unroll
            for (int xp = 0; xp < ST_X / 2; ++xp) {
                const float b = brow[xp * 2];
#pragma unroll
                for (int m = 0; m < MB; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[xp * 2 * COUT + m * 32], b, acc[m], 0, 0, 0);
            }
        }
    }
    if (col_ok) {
        float* out = p.part + (int64_t)blockIdx.x * COUT * ncol;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = m * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
                out[row * ncol + col] = acc[m][i];
            }
    }
}

// part [S][n] fp32 -> grp [SB_GROUPS][n] fp64: group g adds its run of consecutive splits in split order
__global__ void __launch_bounds__(256) stem_mc_bwd_fold_kernel(const float* __restrict__ part, int S, int per, int n,
                                                               double* __restrict__ grp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int s0 = blockIdx.y * per, s1 = min(S, s0 + per);
    double a = 0.0;
    for (int s = s0; s < s1; ++s) a += (double)part[(int64_t)s * n + e];
    grp[(int64_t)blockIdx.y * n + e] = a;
}

// one block: the groups in order (fp64), then the three formulas; the sums over (o, t) per channel go through LDS in a
// fixed order
__global__ void __launch_bounds__(256) stem_mc_bwd_finalize_kernel(const double* __restrict__ grp, int Cin, int Cout,
                                                                   const float* __restrict__ w, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, float* __restrict__ dW,
                                                                   float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double red[256][8];
    const int t = threadIdx.x;
    const int ncol = 27 * (Cin + 1), n = Cout * ncol;
    const double mu = (double)mean[0];
    double dg[4] = {0.0, 0.0, 0.0, 0.0}, db[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < Cout * Cin * 27; i += 256) {
        const int o = i / (Cin * 27), r = i - o * (Cin * 27);
        const int c = r / 27, tp = r - c * 27;
        const int eq = o * ncol + r, es = o * ncol + Cin * 27 + tp;
        double q = 0.0, s = 0.0;
        for (int g = 0; g < SB_GROUPS; ++g) {
            q += grp[(int64_t)g * n + eq];
            s += grp[(int64_t)g * n + es];
        }
        dW[i] = (float)((double)scale[c] * q + (double)shift[c] * s);
        const double wv = (double)w[i];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == c) {
                dg[k] += wv * (q - mu * s);
                db[k] += wv * s;
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        red[t][k] = dg[k];
        red[t][4 + k] = db[k];
    }
    __syncthreads();
    if (t < 2 * Cin) {
        const int c = t % Cin, which = t / Cin;
        double a = 0.0;
        for (int j = 0; j < 256; ++j) a += red[j][which * 4 + c];
        if (which == 0)
            dgamma[c] = (float)((double)rstd[0] * a);
        else
            dbeta[c] = (float)a;
    }
}

struct SbPlan {
    int nby, nbx, ntiles, S, per;
};

static SbPlan sb_plan(int D, int H, int W) {
    SbPlan pl;
    pl.nby = bfm_cdiv(H, ST_Y);
    pl.nbx = bfm_cdiv(W, ST_X);
    const int64_t nt = (int64_t)bfm_cdiv(D, ST_Z) * pl.nby * pl.nbx;
    pl.ntiles = (int)nt;
    const int per_wg = bfm_cdiv(pl.ntiles, std::min(pl.ntiles, SB_MAX_SPLITS));
    pl.S = bfm_cdiv(pl.ntiles, per_wg);                     // every workgroup has a tile
    pl.per = bfm_cdiv(pl.S, SB_GROUPS);
    return pl;
}

static bool sb_shape_ok(int Cin, int Cout, int D, int H, int W) {
    if (Cin < 2 || Cin > 4 || (Cout != 32 && Cout != 64) || D < 1 || H < 1 || W < 1) return false;
    return (int64_t)D * H * W < ((int64_t)1 << 31);        // voxel and tile indices are ints
}

static size_t sb_part_bytes(int Cin, int Cout, int S) {
    return (((size_t)S * Cout * 27 * (Cin + 1) * sizeof(float)) + 255) & ~(size_t)255;
}

}  // namespace

extern "C" size_t bfm_stem_mc_bwd_workspace(int Cin, int Cout, int D, int H, int W) {
    if (!sb_shape_ok(Cin, Cout, D, H, W)) return 0;
    const SbPlan pl = sb_plan(D, H, W);
    return sb_part_bytes(Cin, Cout, pl.S) + (size_t)SB_GROUPS * Cout * 27 * (Cin + 1) * sizeof(double);
}

extern "C" int bfm_stem_mc_bwd(const float* dP, int Cout, const float* x, int Cin, int D, int H, int W, const float* w_raw,
                               const float* scale, const float* shift, const float* mean, const float* rstd, float* dW,
                               float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (!dP || !x || !w_raw || !scale || !shift || !mean || !rstd || !dW || !dgamma || !dbeta || !workspace) return BFM_E_ARG;
    if (!sb_shape_ok(Cin, Cout, D, H, W)) return BFM_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(dP) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return BFM_E_ARG;
    if (workspace_bytes < bfm_stem_mc_bwd_workspace(Cin, Cout, D, H, W)) return BFM_E_WORKSPACE;
    const SbPlan pl = sb_plan(D, H, W);
    StemBwdParams p{};
    p.dP = dP; p.x = x; p.Cin = Cin; p.D = D; p.H = H; p.W = W;
    p.nby = pl.nby; p.nbx = pl.nbx; p.ntiles = pl.ntiles;
    p.part = static_cast<float*>(workspace);
    double* grp = reinterpret_cast<double*>(static_cast<char*>(workspace) + sb_part_bytes(Cin, Cout, pl.S));
    hipStream_t st = bfm_s(stream);
    const int ncol = 27 * (Cin + 1), n = Cout * ncol;
    const int threads = 64 * bfm_cdiv(ncol, 32);            // 192 / 256 / 320: one wave per 32 columns
    const int lds = sb_lds_bytes(Cin, Cout);
    static bool attr32 = false, attr64 = false;
    if (Cout == 32) {
        if (!attr32) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_mc_bwd_kernel<32>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, sb_lds_bytes(4, 32)) != hipSuccess)
                return BFM_E_LAUNCH;
            attr32 = true;
        }
        hipLaunchKernelGGL(stem_mc_bwd_kernel<32>, dim3(pl.S), dim3(threads), lds, st, p);
    } else {
        if (!attr64) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_mc_bwd_kernel<64>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, sb_lds_bytes(4, 64)) != hipSuccess)
                return BFM_E_LAUNCH;
            attr64 = true;
        }
        hipLaunchKernelGGL(stem_mc_bwd_kernel<64>, dim3(pl.S), dim3(threads), lds, st, p);
    }
    hipLaunchKernelGGL(stem_mc_bwd_fold_kernel, dim3(bfm_cdiv(n, 256), SB_GROUPS), dim3(256), 0, st, p.part, pl.S, pl.per, n, grp);
    hipLaunchKernelGGL(stem_mc_bwd_finalize_kernel, dim3(1), dim3(256), 0, st, grp, Cin, Cout, w_raw, scale, shift, mean, rstd,
                       dW, dgamma, dbeta);
    return bfm_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------------
// Input gradient of the same layer with respect to ONE input channel c, and its chain through the masking of the two-stage
// model into the stage-0 logit (Trainer/engine.py:238: input_masked = input * (1 - sigmoid(raw0)); torch autograd over
// buildingblocks.py:31-60).  With xhat = (X - mean) rstd, N = Cin D H W:
//
//     G_c[u]  = sum_{o,k} dP[u - k + 1, o] W[o, c, k]                      (zero outside the volume)
//     dX_c[u] = rstd (gamma_c G_c[u] - m1 - xhat_c[u] m2),   m1 = sum_c' gamma_c' dbeta_c' / N,  m2 = sum_c' gamma_c' dgamma_c' / N
//     dRaw[col_offset + u voxel_stride] += -x_raw[u] dX_c[u] p[u] (1 - p[u])
//
// The group sums are the dgamma / dbeta the parameter backward has already produced, so only channel c's G is formed: one
// launch, no reduction pass, no dXn tensor.
//
// stem_mc_dgrad_kernel<COUT>: workgroups over 4x4x16-voxel tiles.  Per tile, T[v, k] = sum_o dP[v, o] W[o, c, k] over the
// tile's voxels and their one-voxel halo (648 voxels) is a GEMM M = 648 (21 blocks of 32), K = COUT, N = 27 of 32 on the
// exact-fp32 matrix core.  The A operand comes straight from HBM: lane (l32, lh) reads the COUT / 2 consecutive channels
// lh COUT / 2 .. of voxel l32 (the order of the K steps is free, so the two lane halves take the two halves of a voxel's
// row), the B operand (this channel's weights) stays in registers.  T goes to LDS as [tap][voxel] (odd pitch), and
// G[u] = sum_k T[k][u - k + 1] is 27 LDS reads per lane in tap order.  One writer per voxel, no atomics: the same bits on
// every run.
namespace {

constexpr int DG_TP = SH_VOX + 1;                           // odd pitch: a wave's 27 taps of one voxel hit different banks
constexpr int DG_MB = (SH_VOX + 31) / 32;                   // 21
constexpr int DG_THREADS = ST_VOX;                          // one lane per tile voxel in the second phase

// the mask chain of one voxel: bfm_stem_mc_dgrad's epilogue and bfm_mask_chain_bwd share the expression (and its bits)
__device__ __forceinline__ float mask_chain_term(float xr, float dx, float p) {
    const float a = -xr * dx;
    const float b = a * p;
    return b * (1.f - p);
}

struct StemDgradParams {
    const float* dP;                  // [D][H][W][COUT]
    const float* x;                   // [D][H][W][Cin]
    const float* w;                   // [COUT][Cin][27]
    const float *gamma, *mean, *rstd, *dgamma, *dbeta;
    int Cin, D, H, W, channel;
    int nby, nbx, ntiles;
    float* dx;                        // [D][H][W] or NULL
    const float *x_raw, *p;           // [D][H][W] each, or both NULL
    float* dRaw;
    int64_t col_offset, voxel_stride;
};

template <int COUT>
__global__ void __launch_bounds__(DG_THREADS) stem_mc_dgrad_kernel(const StemDgradParams q) {
    extern __shared__ float Ts[];                           // [27][DG_TP]
    constexpr int HALF = COUT / 2;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, l32 = lane & 31, lh = lane >> 5;
    const int c = q.channel;
    // B[k = (lh, j)][n = l32] = W[o = lh HALF + j][c][tap l32]
    float breg[HALF];
#pragma unroll
    for (int j = 0; j < HALF; ++j)
        breg[j] = l32 < 27 ? q.w[((lh * HALF + j) * q.Cin + c) * 27 + l32] : 0.f;
    // the two group means of the GroupNorm backward, from the parameter gradients
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < q.Cin; ++k) {
        s1 += (double)q.gamma[k] * (double)q.dbeta[k];
        s2 += (double)q.gamma[k] * (double)q.dgamma[k];
    }
    const double nrm = (double)q.Cin * (double)q.D * (double)q.H * (double)q.W;
    const float m1 = (float)(s1 / nrm), m2 = (float)(s2 / nrm);
    const float mean = q.mean[0], rstd = q.rstd[0], gam = q.gamma[c];
    const int zl = tid >> 6, yl = (tid >> 4) & 3, xl = tid & 15;

    for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
        const int bx = tile % q.nbx;
        const int t2 = tile / q.nbx;
        const int by = t2 % q.nby, bz = t2 / q.nby;
        const int z0 = bz * ST_Z, y0 = by * ST_Y, x0 = bx * ST_X;
        __syncthreads();                                    // the previous tile's reads of Ts are done
        for (int mb = wave; mb < DG_MB; mb += DG_THREADS / 64) {
            const int hv = mb * 32 + l32;
            const int hz = hv / (SH_Y * SH_X);
            const int r = hv - hz * (SH_Y * SH_X);
            const int hy = r / SH_X, hx = r - hy * SH_X;
            const int zz = z0 + hz - 1, yy = y0 + hy - 1, xx = x0 + hx - 1;
            const bool in = hv < SH_VOX && zz >= 0 && zz < q.D && yy >= 0 && yy < q.H && xx >= 0 && xx < q.W;
            float4 a[HALF / 4];
            if (in) {
                const float4* src = reinterpret_cast<const float4*>(q.dP + ((int64_t)(zz * q.H + yy) * q.W + xx) * COUT + lh * HALF);
#pragma unroll
                for (int j = 0; j < HALF / 4; ++j) a[j] = src[j];
            } else {
#pragma unroll
                for (int j = 0; j < HALF / 4; ++j) a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            floatx16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int j = 0; j < HALF / 4; ++j) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, breg[4 * j + 0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, breg[4 * j + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, breg[4 * j + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, breg[4 * j + 3], acc, 0, 0, 0);
            }
            if (l32 < 27) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = mb * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
                    if (row < SH_VOX) Ts[l32 * DG_TP + row] = acc[i];
                }
            }
        }
        __syncthreads();
        const int z = z0 + zl, y = y0 + yl, x = x0 + xl;
        if (z < q.D && y < q.H && x < q.W) {
            float g = 0.f;
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                const int kd = k / 9, kh = (k / 3) % 3, kw = k % 3;
                g += Ts[k * DG_TP + ((zl + 2 - kd) * SH_Y + (yl + 2 - kh)) * SH_X + (xl + 2 - kw)];
            }
            const int64_t u = (int64_t)(z * q.H + y) * q.W + x;
            const float xhat = (q.x[u * q.Cin + c] - mean) * rstd;
            const float dxv = rstd * (gam * g - m1 - xhat * m2);
            if (q.dx) q.dx[u] = dxv;
            if (q.p) {
                const int64_t o = q.col_offset + u * q.voxel_stride;
                q.dRaw[o] += mask_chain_term(q.x_raw[u], dxv, q.p[u]);
            }
        }
    }
}

__global__ void __launch_bounds__(256) mask_chain_bwd_kernel(const float* __restrict__ dx, int64_t dx_stride,
                                                             const float* __restrict__ x_raw, const float* __restrict__ p,
                                                             int64_t n, float* __restrict__ dRaw, int64_t col_offset,
                                                             int64_t voxel_stride) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n; u += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = col_offset + u * voxel_stride;
        dRaw[o] += mask_chain_term(x_raw[u], dx[u * dx_stride], p[u]);
    }
}

}  // namespace

extern "C" int bfm_stem_mc_dgrad(const float* dP, int Cout, const float* x_cl, int Cin, int D, int H, int W, const float* w_raw,
                                 const float* gamma, const float* mean, const float* rstd, const float* dgamma,
                                 const float* dbeta, int channel, float* dx, const float* x_raw, const float* p, float* dRaw,
                                 int64_t col_offset, int64_t voxel_stride, bfm_stream_t stream) {
    if (!dP || !x_cl || !w_raw || !gamma || !mean || !rstd || !dgamma || !dbeta) return BFM_E_ARG;
    const bool chain = x_raw || p;
    if (chain && (!x_raw || !p || !dRaw || col_offset < 0 || voxel_stride < 1)) return BFM_E_ARG;
    if (!chain && !dx) return BFM_E_ARG;                    // nothing to write
    if (!sb_shape_ok(Cin, Cout, D, H, W) || channel < 0 || channel >= Cin) return BFM_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(dP) & 15) return BFM_E_ARG;
    const SbPlan pl = sb_plan(D, H, W);
    StemDgradParams q{};
    q.dP = dP; q.x = x_cl; q.w = w_raw; q.gamma = gamma; q.mean = mean; q.rstd = rstd; q.dgamma = dgamma; q.dbeta = dbeta;
    q.Cin = Cin; q.D = D; q.H = H; q.W = W; q.channel = channel;
    q.nby = pl.nby; q.nbx = pl.nbx; q.ntiles = pl.ntiles;
    q.dx = dx; q.x_raw = x_raw; q.p = p; q.dRaw = dRaw; q.col_offset = col_offset; q.voxel_stride = voxel_stride;
    const int grid = std::min(pl.ntiles, 4096);
    constexpr int lds = 27 * DG_TP * (int)sizeof(float);    // 70 KB: above the static limit
    // the attribute belongs to the device: one flag per device and kernel (setting it twice is harmless)
    static bool attr[2][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return BFM_E_LAUNCH;
    const int wide = Cout == 64 ? 1 : 0;
    const void* fn = wide ? reinterpret_cast<const void*>(&stem_mc_dgrad_kernel<64>)
                          : reinterpret_cast<const void*>(&stem_mc_dgrad_kernel<32>);
    if (dev < 0 || dev >= 64 || !attr[wide][dev]) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return BFM_E_LAUNCH;
        if (dev >= 0 && dev < 64) attr[wide][dev] = true;
    }
    if (wide)
        hipLaunchKernelGGL(stem_mc_dgrad_kernel<64>, dim3(grid), dim3(DG_THREADS), lds, bfm_s(stream), q);
    else
        hipLaunchKernelGGL(stem_mc_dgrad_kernel<32>, dim3(grid), dim3(DG_THREADS), lds, bfm_s(stream), q);
    return bfm_launch_status();
}

extern "C" int bfm_mask_chain_bwd(const float* dx, int64_t dx_stride, const float* x_raw, const float* p, int64_t n, float* dRaw,
                                  int64_t col_offset, int64_t voxel_stride, bfm_stream_t stream) {
    if (!dx || !x_raw || !p || !dRaw || n <= 0 || dx_stride < 1 || col_offset < 0 || voxel_stride < 1) return BFM_E_ARG;
    const int grid = (int)std::min<int64_t>(bfm_cdiv64(n, 256), 4096);
    hipLaunchKernelGGL(mask_chain_bwd_kernel, dim3(grid), dim3(256), 0, bfm_s(stream), dx, dx_stride, x_raw, p, n, dRaw,
                       col_offset, voxel_stride);
    return bfm_launch_status();
}
