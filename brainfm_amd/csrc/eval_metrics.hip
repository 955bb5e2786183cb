// The evaluator's device arithmetic: Trainer/models/evaluator.py (Evaluator.get_dice / get_l1 / get_psnr / get_normalized_l2 /
// get_ssim / get_ms_ssim, get_onehot + get_dice for label maps) on volumes that are already resident after inference.
//
//   pair_stats     one read of o and t -> ten fp64 numbers; L1, MSE, PSNR and the normalised L2 are host arithmetic on them
//   l1_nonzero     get_l1(nonzero_only=True): the reference sums over dim 0 (the batch), so the result is a volume
//   channel_sums   soft Dice: per (b, c) plane sum(o t) and sum(o + t)
//   label_counts   Dice of two label maps without the one-hot: |P_l|, |T_l|, |P_l & T_l| per class (integers)
//   ssim3d         SSIM / contrast-structure means of pytorch_msssim's 3-D form, fused: no filtered moment leaves the CU
//   avgpool2_pair  the 2x average pooling between MS-SSIM scales, both volumes in one launch
//
// Reductions: every lane sums in fp64, a block folds its lanes in a fixed tree, fold_kernel folds the block partials in an
// order that depends on their number alone -- no float atomics, the same bits on every run.  label_counts adds integers
// (LDS histogram, then global integer adds), which is exact in any order.
//
// ssim3d.  Volumes are (D, H, W), W contiguous.  A block of 256 lanes owns an 8 (H) x 32 (W) tile of output voxels and a
// chunk of output planes along D, and walks the chunk's input planes once.  Per input plane: the (8+10) x (32+10) windows of
// X and Y go to LDS (min/max normalised on the way in), the W pass of the five products X, Y, XX, YY, XY goes LDS -> LDS
// (18 rows x 32), the H pass LDS -> 5 registers per lane, and the D pass scatters those five values with the eleven weights
// into 11 x 5 running sums; the loop over input planes is unrolled 11 times so the ring of running sums is compile-time
// register naming.  The output plane that just received its last tap goes through the SSIM expression into the lane's two
// fp64 sums.  An axis shorter than the window is not filtered (pytorch_msssim skips it): the same kernel with that pass a
// one-tap identity (template flags).  The next plane's global loads are issued before the W pass of the current one.
#include "bfm_common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 1024;
constexpr int LABEL_BLOCKS = 512;                            // every block ends with up to 3 n_labels + 1 global adds to the same words
constexpr int NSTAT = 10;                                    // bfm_eval_pair_stats' outputs
constexpr int MAX_LABELS = 256;

// torch.min / torch.max propagate NaN
__device__ __forceinline__ float nan_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ double nan_min(double m, double v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ double block_sum(double v, double* red) {          // NT threads, fixed tree
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}
// mode 0 sum, 1 min, 2 max
__device__ __forceinline__ double comb(double a, double b, int mode) {
    return mode == 0 ? a + b : (mode == 1 ? nan_min(a, b) : nan_max(a, b));
}
constexpr int FOLD_MAXK = 10;                                // values per partial row (bfm_eval_pair_stats has the most)

// Block blockIdx.x folds its nb rows of nk <= FOLD_MAXK partials: a lane takes rows lane, lane + 256, ... in that order (a
// row's nk loads are independent, so they are in flight together), a wave folds its lanes by xor-shuffles, the four waves are
// folded in order: out[blockIdx.x][k] = fold_i part[blockIdx.x][i][k]  (sums times `scale`; bits of min_mask / max_mask pick
// min / max).  The order depends on nb alone: the same bits on every run.
__global__ void __launch_bounds__(NT) fold_kernel(const double* __restrict__ part, int nb, int nk, unsigned min_mask,
                                                  unsigned max_mask, double scale, double* __restrict__ out) {
    __shared__ double red[NT / BFM_WAVE][FOLD_MAXK];
    const double* p = part + (int64_t)blockIdx.x * nb * nk;
    int mode[FOLD_MAXK];
    double v[FOLD_MAXK];
#pragma unroll
    for (int k = 0; k < FOLD_MAXK; ++k) {
        mode[k] = (min_mask >> k & 1u) ? 1 : ((max_mask >> k & 1u) ? 2 : 0);
        v[k] = mode[k] == 0 ? 0.0 : (mode[k] == 1 ? (double)INFINITY : -(double)INFINITY);
    }
    for (int i = threadIdx.x; i < nb; i += NT) {
        const double* r = p + (int64_t)i * nk;
#pragma unroll
        for (int k = 0; k < FOLD_MAXK; ++k)
            if (k < nk) v[k] = comb(v[k], r[k], mode[k]);
    }
#pragma unroll
    for (int k = 0; k < FOLD_MAXK; ++k) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[k] = comb(v[k], __shfl_xor(v[k], s, BFM_WAVE), mode[k]);
        if ((threadIdx.x & (BFM_WAVE - 1)) == 0) red[threadIdx.x / BFM_WAVE][k] = v[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < nk) {
        const int k = threadIdx.x;
        const int m = (min_mask >> k & 1u) ? 1 : ((max_mask >> k & 1u) ? 2 : 0);
        double r = red[0][k];
        for (int w = 1; w < NT / BFM_WAVE; ++w) r = comb(r, red[w][k], m);
        out[(int64_t)blockIdx.x * nk + k] = m == 0 ? r * scale : r;
    }
}

// ------------------------------------------------------------------------------------------------ pair statistics
static_assert(NSTAT <= FOLD_MAXK, "fold_kernel holds a partial row in registers");
struct PairAcc {
    double sad, ssd, sot, soo, stt, nz;
    float mno, mxo, mnt, mxt;
};

__device__ __forceinline__ void pair_add(PairAcc& a, float o, float t) {
    const double od = (double)o, td = (double)t, d = od - td;
    a.sad += fabs(d);
    a.ssd += d * d;
    a.sot += od * td;
    a.soo += od * od;
    a.stt += td * td;
    a.nz += t != 0.f ? 1.0 : 0.0;
    a.mno = nan_min(a.mno, o); a.mxo = nan_max(a.mxo, o);
    a.mnt = nan_min(a.mnt, t); a.mxt = nan_max(a.mxt, t);
}

__device__ __forceinline__ int pair_mode(int k) { return (k == 5 || k == 7) ? 1 : ((k == 6 || k == 8) ? 2 : 0); }

__global__ void __launch_bounds__(NT) pair_stats_kernel(const float* __restrict__ o, const float* __restrict__ t, int64_t n,
                                                        int vec, double* __restrict__ part) {
    __shared__ double red[NT / BFM_WAVE][NSTAT];
    PairAcc a{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY, INFINITY, -INFINITY};
    const int64_t stride = (int64_t)gridDim.x * NT, i0 = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int64_t n4 = vec ? n / 4 : 0;
    const float4* o4 = reinterpret_cast<const float4*>(o);
    const float4* t4 = reinterpret_cast<const float4*>(t);
    int64_t i = i0;
    for (; i + stride < n4; i += 2 * stride) {               // four 16-byte loads in flight per lane
        const float4 p0 = o4[i], q0 = t4[i], p1 = o4[i + stride], q1 = t4[i + stride];
        pair_add(a, p0.x, q0.x); pair_add(a, p0.y, q0.y); pair_add(a, p0.z, q0.z); pair_add(a, p0.w, q0.w);
        pair_add(a, p1.x, q1.x); pair_add(a, p1.y, q1.y); pair_add(a, p1.z, q1.z); pair_add(a, p1.w, q1.w);
    }
    if (i < n4) {
        const float4 p = o4[i], q = t4[i];
        pair_add(a, p.x, q.x); pair_add(a, p.y, q.y); pair_add(a, p.z, q.z); pair_add(a, p.w, q.w);
    }
    for (int64_t j = n4 * 4 + i0; j < n; j += stride) pair_add(a, o[j], t[j]);
    double v[NSTAT] = {a.sad, a.ssd, a.sot, a.soo, a.stt, (double)a.mno, (double)a.mxo, (double)a.mnt, (double)a.mxt, a.nz};
    // lanes of a wave by xor-shuffles, then the block's four waves in order: a fixed tree
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[k] = comb(v[k], __shfl_xor(v[k], s, BFM_WAVE), pair_mode(k));
        if ((threadIdx.x & (BFM_WAVE - 1)) == 0) red[threadIdx.x / BFM_WAVE][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NSTAT) {
        const int k = threadIdx.x;
        double r = red[0][k];
        for (int w = 1; w < NT / BFM_WAVE; ++w) r = comb(r, red[w][k], pair_mode(k));
        part[(int64_t)blockIdx.x * NSTAT + k] = r;
    }
}

__global__ void __launch_bounds__(NT) l1_nonzero_kernel(const float* __restrict__ o, const float* __restrict__ t, int B,
                                                        int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        float num = 0.f, den = 0.f;
        for (int b = 0; b < B; ++b) {
            const float tv = t[(int64_t)b * n + i], ov = o[(int64_t)b * n + i];
            const float m = tv != 0.f ? 1.f : 0.f;
            num += fabsf(tv - ov) * m;                       // NaN * 0 stays NaN, as in the reference
            den += m;
        }
        out[i] = num / den;                                  // 0 / 0 = NaN where no sample has a non-zero target
    }
}

// ------------------------------------------------------------------------------------------------ soft Dice sums
__global__ void __launch_bounds__(NT) channel_sums_kernel(const float* __restrict__ o, const float* __restrict__ t,
                                                          int64_t n, double* __restrict__ part) {
    __shared__ double red[NT];
    const float* op = o + (int64_t)blockIdx.y * n;
    const float* tp = t + (int64_t)blockIdx.y * n;
    double sp = 0.0, ss = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const double a = (double)op[i], b = (double)tp[i];
        sp += a * b;
        ss += a + b;
    }
    const double r0 = block_sum(sp, red);
    const double r1 = block_sum(ss, red);
    if (threadIdx.x == 0) {
        double* p = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = r0; p[1] = r1;
    }
}

// ------------------------------------------------------------------------------------------------ label counts
struct LabelAcc { unsigned p0, t0, i0, bad; };

// One count into LDS bin idx (-1: none).  Inside an anatomical structure every lane of a wave hits the same bin, which an LDS
// atomic would take one lane at a time: when the active lanes agree, the first of them adds their number instead.
__device__ __forceinline__ void hist_add(unsigned* h, int idx) {
    const unsigned long long act = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(idx);
    if (__ballot(idx == first) == act) {
        if (idx >= 0 && (int)(threadIdx.x & (BFM_WAVE - 1)) == __ffsll((long long)act) - 1)
            atomicAdd(&h[idx], (unsigned)__popcll(act));
    } else if (idx >= 0) {
        atomicAdd(&h[idx], 1u);
    }
}

__device__ __forceinline__ void label_add(LabelAcc& a, int p, int t, const int32_t* __restrict__ lut, int nlut, int nl,
                                          unsigned* h) {
    int cp = (unsigned)p < (unsigned)nlut ? lut[p] : -1;
    int ct = (unsigned)t < (unsigned)nlut ? lut[t] : -1;
    if ((unsigned)cp >= (unsigned)nl) cp = -1;               // keeps every histogram index inside [0, 3 nl]
    if ((unsigned)ct >= (unsigned)nl) ct = -1;
    a.bad += (cp < 0) + (ct < 0);
    // class 0 (background, most of a brain volume) is counted in registers
    a.p0 += cp == 0;
    a.t0 += ct == 0;
    a.i0 += cp == 0 && ct == 0;
    hist_add(h, cp > 0 ? cp : -1);
    hist_add(h, ct > 0 ? nl + ct : -1);
    hist_add(h, (cp > 0 && cp == ct) ? 2 * nl + cp : -1);
}

__global__ void __launch_bounds__(NT) label_counts_kernel(const int32_t* __restrict__ P, const int32_t* __restrict__ T,
                                                          int64_t n, int vec, const int32_t* __restrict__ lut, int nlut,
                                                          int nl, unsigned long long* __restrict__ counts) {
    __shared__ unsigned h[3 * MAX_LABELS + 1];
    const int nh = 3 * nl + 1;
    for (int i = threadIdx.x; i < nh; i += NT) h[i] = 0u;
    __syncthreads();
    LabelAcc a{0u, 0u, 0u, 0u};
    const int64_t stride = (int64_t)gridDim.x * NT, i0 = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int64_t n4 = vec ? n / 4 : 0;
    const int4* P4 = reinterpret_cast<const int4*>(P);
    const int4* T4 = reinterpret_cast<const int4*>(T);
    int64_t i = i0;
    for (; i + stride < n4; i += 2 * stride) {               // four 16-byte loads in flight per lane
        const int4 p0 = P4[i], q0 = T4[i], p1 = P4[i + stride], q1 = T4[i + stride];
        label_add(a, p0.x, q0.x, lut, nlut, nl, h); label_add(a, p0.y, q0.y, lut, nlut, nl, h);
        label_add(a, p0.z, q0.z, lut, nlut, nl, h); label_add(a, p0.w, q0.w, lut, nlut, nl, h);
        label_add(a, p1.x, q1.x, lut, nlut, nl, h); label_add(a, p1.y, q1.y, lut, nlut, nl, h);
        label_add(a, p1.z, q1.z, lut, nlut, nl, h); label_add(a, p1.w, q1.w, lut, nlut, nl, h);
    }
    if (i < n4) {
        const int4 p = P4[i], q = T4[i];
        label_add(a, p.x, q.x, lut, nlut, nl, h); label_add(a, p.y, q.y, lut, nlut, nl, h);
        label_add(a, p.z, q.z, lut, nlut, nl, h); label_add(a, p.w, q.w, lut, nlut, nl, h);
    }
    for (int64_t j = n4 * 4 + i0; j < n; j += stride) label_add(a, P[j], T[j], lut, nlut, nl, h);
    if (a.p0) atomicAdd(&h[0], a.p0);
    if (a.t0) atomicAdd(&h[nl], a.t0);
    if (a.i0) atomicAdd(&h[2 * nl], a.i0);
    if (a.bad) atomicAdd(&h[3 * nl], a.bad);
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += NT)
        if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
}

// ------------------------------------------------------------------------------------------------ SSIM
constexpr int KW = 11, HALO = KW - 1;
constexpr int TY = 8, TZ = 32;                               // output tile: 8 rows (H) x 32 columns (W) = one voxel per lane
constexpr int SSIM_TARGET_BLOCKS = 1024, SSIM_MIN_CHUNK = 4;

struct SsimWin { float g[KW]; };
struct SsimPlan { int Do, Ho, Wo, tiles, nchunk, chunk; };

inline SsimPlan ssim_plan(int planes, int D, int H, int W) {
    SsimPlan p;
    p.Do = D >= KW ? D - HALO : D;
    p.Ho = H >= KW ? H - HALO : H;
    p.Wo = W >= KW ? W - HALO : W;
    p.tiles = bfm_cdiv(p.Ho, TY) * bfm_cdiv(p.Wo, TZ);
    // chunks along D: enough blocks to fill the chip, each chunk re-reads 10 planes of halo
    const int64_t have = (int64_t)p.tiles * planes;
    int want = (int)std::min<int64_t>(bfm_cdiv64(SSIM_TARGET_BLOCKS, have), bfm_cdiv(p.Do, SSIM_MIN_CHUNK));
    want = std::max(1, want);
    p.chunk = bfm_cdiv(p.Do, want);
    p.nchunk = bfm_cdiv(p.Do, p.chunk);
    return p;
}

template <bool FX, bool FY, bool FZ>
__global__ void __launch_bounds__(NT) ssim3d_kernel(const float* __restrict__ X, const float* __restrict__ Y, int D, int H,
                                                    int W, SsimPlan pl, SsimWin win, const double* __restrict__ norm,
                                                    double* __restrict__ part) {
    constexpr int IY = TY + (FY ? HALO : 0), IZ = TZ + (FZ ? HALO : 0);
    constexpr int NY = FY ? KW : 1, NZ = FZ ? KW : 1;
    constexpr int NE = IY * IZ, PER = (NE + NT - 1) / NT;
    __shared__ float tx[NE], ty[NE];
    __shared__ float zb[5][IY * TZ];
    __shared__ double red[NT];

    const int tid = threadIdx.x;
    const int ntz = bfm_cdiv(pl.Wo, TZ);
    const int y0 = ((int)blockIdx.x / ntz) * TY, z0 = ((int)blockIdx.x % ntz) * TZ;
    const int o0 = (int)blockIdx.y * pl.chunk, o1 = min(pl.Do, o0 + pl.chunk);
    const int nin = (o1 - o0) + (FX ? HALO : 0);             // input planes o0 .. o0 + nin - 1 (< D by construction)
    const int64_t hw = (int64_t)H * W;
    const float* Xp = X + (int64_t)blockIdx.z * D * hw;
    const float* Yp = Y + (int64_t)blockIdx.z * D * hw;
    float lox = 0.f, rx = 1.f, loy = 0.f, ry = 1.f;
    if (norm) {                                              // (x - min) / (max - min), a true division, on load
        lox = (float)norm[0]; rx = (float)norm[1] - lox;
        loy = (float)norm[2]; ry = (float)norm[3] - loy;
    }
    const int ly = tid / TZ, lz = tid % TZ;
    const bool valid = y0 + ly < pl.Ho && z0 + lz < pl.Wo;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

    // this lane's elements of a staged window: offsets inside a plane, -1 outside the volume (read as zero; such elements
    // only reach output voxels outside the valid range)
    int off[PER];
#pragma unroll
    for (int m = 0; m < PER; ++m) {
        const int e = tid + m * NT;
        const int r = e / IZ, c = e - r * IZ;
        off[m] = (e < NE && y0 + r < H && z0 + c < W) ? (y0 + r) * W + (z0 + c) : -1;
    }
    float px[PER], py[PER];
    auto fetch = [&](int plane) {
        const int64_t base = (int64_t)plane * hw;
#pragma unroll
        for (int m = 0; m < PER; ++m) {
            px[m] = off[m] >= 0 ? Xp[base + off[m]] : 0.f;
            py[m] = off[m] >= 0 ? Yp[base + off[m]] : 0.f;
        }
    };

    float acc[KW][5];
#pragma unroll
    for (int s = 0; s < KW; ++s)
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[s][j] = 0.f;
    double s_ssim = 0.0, s_cs = 0.0;

    auto finish = [&](const float (&v)[5]) {
        const float mu1 = v[0], mu2 = v[1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float sigma1_sq = v[2] - mu1_sq, sigma2_sq = v[3] - mu2_sq, sigma12 = v[4] - mu1_mu2;
        const float cs = (2.f * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2);
        const float ss = ((2.f * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs;
        if (valid) { s_ssim += (double)ss; s_cs += (double)cs; }
    };

    fetch(o0);
    for (int base = 0; base < nin; base += KW) {
#pragma unroll
        for (int u = 0; u < KW; ++u) {
            const int li = base + u;
            if (li >= nin) break;                            // the same for every lane of the block
#pragma unroll
            for (int m = 0; m < PER; ++m) {
                const int e = tid + m * NT;
                if (e < NE) {
                    const bool in = off[m] >= 0;
                    tx[e] = in ? (px[m] - lox) / rx : 0.f;
                    ty[e] = in ? (py[m] - loy) / ry : 0.f;
                }
            }
            __syncthreads();
            if (li + 1 < nin) fetch(o0 + li + 1);            // in flight during the W and H passes
            for (int i = tid; i < IY * TZ; i += NT) {        // W pass
                const int r = i / TZ, c = i - r * TZ;
                const float* a = tx + r * IZ + c;
                const float* b = ty + r * IZ + c;
                float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
                for (int k = 0; k < NZ; ++k) {
                    const float w = FZ ? win.g[k] : 1.f, xv = a[k], yv = b[k];
                    sx = fmaf(w, xv, sx); sy = fmaf(w, yv, sy);
                    sxx = fmaf(w, xv * xv, sxx); syy = fmaf(w, yv * yv, syy); sxy = fmaf(w, xv * yv, sxy);
                }
                zb[0][i] = sx; zb[1][i] = sy; zb[2][i] = sxx; zb[3][i] = syy; zb[4][i] = sxy;
            }
            __syncthreads();
            float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};          // H pass
#pragma unroll
            for (int k = 0; k < NY; ++k) {
                const float w = FY ? win.g[k] : 1.f;
#pragma unroll
                for (int j = 0; j < 5; ++j) v[j] = fmaf(w, zb[j][(ly + k) * TZ + lz], v[j]);
            }
            if (FX) {                                        // D pass: output plane o (local) lives in slot o % 11
#pragma unroll
                for (int s = 0; s < KW; ++s) {
                    const float w = win.g[(u - s + KW) % KW];
#pragma unroll
                    for (int j = 0; j < 5; ++j) acc[s][j] = fmaf(w, v[j], acc[s][j]);
                }
                const int sdone = (u + 1) % KW;              // local output li - 10 has all eleven taps now
                if (li >= HALO) finish(acc[sdone]);
#pragma unroll
                for (int j = 0; j < 5; ++j) acc[sdone][j] = 0.f;
            } else {
                finish(v);
            }
        }
    }
    const double r0 = block_sum(s_ssim, red);
    const double r1 = block_sum(s_cs, red);
    if (tid == 0) {
        double* p = part + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
        p[0] = r0; p[1] = r1;
    }
}

// F.avg_pool3d(kernel 2, padding n % 2 per axis, count_include_pad): window i of an odd axis covers inputs 2i-1 and 2i
__global__ void __launch_bounds__(NT) avgpool2_pair_kernel(const float* __restrict__ X, const float* __restrict__ Y, int D,
                                                           int H, int W, int Dp, int Hp, int Wp, int64_t total,
                                                           const double* __restrict__ norm, float* __restrict__ Xo,
                                                           float* __restrict__ Yo) {
    float lox = 0.f, rx = 1.f, loy = 0.f, ry = 1.f;
    if (norm) {
        lox = (float)norm[0]; rx = (float)norm[1] - lox;
        loy = (float)norm[2]; ry = (float)norm[3] - loy;
    }
    const int pd = D & 1, ph = H & 1, pw = W & 1;
    const int64_t hw = (int64_t)H * W, vol = (int64_t)D * hw, pvol = (int64_t)Dp * Hp * Wp;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int64_t plane = i / pvol;
        int64_t r = i - plane * pvol;
        const int w = (int)(r % Wp); r /= Wp;
        const int h = (int)(r % Hp);
        const int d = (int)(r / Hp);
        const float* xp = X + plane * vol;
        const float* yp = Y + plane * vol;
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int id = 2 * d - pd + a, ih = 2 * h - ph + b, iw = 2 * w - pw + c;
                    if (id >= 0 && id < D && ih >= 0 && ih < H && iw >= 0 && iw < W) {
                        const int64_t q = (int64_t)id * hw + (int64_t)ih * W + iw;
                        sx += norm ? (xp[q] - lox) / rx : xp[q];
                        sy += norm ? (yp[q] - loy) / ry : yp[q];
                    }
                }
        Xo[i] = sx / 8.f;
        Yo[i] = sy / 8.f;
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int stream_blocks(int64_t n) { return (int)std::min<int64_t>(MAX_BLOCKS, bfm_cdiv64(n, (int64_t)NT * 4)); }
inline int channel_blocks(int64_t n_per) { return (int)std::min<int64_t>(64, bfm_cdiv64(n_per, (int64_t)NT * 8)); }

}  // namespace

extern "C" size_t bfm_eval_pair_stats_workspace(void) { return (size_t)MAX_BLOCKS * NSTAT * sizeof(double); }

extern "C" int bfm_eval_pair_stats(const float* o, const float* t, int64_t n, double* stats, void* workspace,
                                   size_t workspace_bytes, bfm_stream_t stream) {
    if (!o || !t || !stats || !workspace || n <= 0 || !aligned8(workspace) || !aligned8(stats)) return BFM_E_ARG;
    if (workspace_bytes < bfm_eval_pair_stats_workspace()) return BFM_E_WORKSPACE;
    double* part = static_cast<double*>(workspace);
    const int nb = stream_blocks(n);
    const int vec = aligned16(o) && aligned16(t);
    hipLaunchKernelGGL(pair_stats_kernel, dim3(nb), dim3(NT), 0, bfm_s(stream), o, t, n, vec, part);
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(NT), 0, bfm_s(stream), part, nb, NSTAT, (1u << 5) | (1u << 7),
                       (1u << 6) | (1u << 8), 1.0, stats);
    return bfm_launch_status();
}

extern "C" int bfm_eval_l1_nonzero(const float* o, const float* t, int B, int64_t n, float* out, bfm_stream_t stream) {
    if (!o || !t || !out || B <= 0 || n <= 0) return BFM_E_ARG;
    hipLaunchKernelGGL(l1_nonzero_kernel, dim3((unsigned)std::min<int64_t>(8192, bfm_cdiv64(n, NT))), dim3(NT), 0,
                       bfm_s(stream), o, t, B, n, out);
    return bfm_launch_status();
}

extern "C" size_t bfm_eval_channel_sums_workspace(int planes, int64_t n_per) {
    if (planes <= 0 || n_per <= 0) return 0;
    return (size_t)planes * channel_blocks(n_per) * 2 * sizeof(double);
}

extern "C" int bfm_eval_channel_sums(const float* o, const float* t, int planes, int64_t n_per, double* out,
                                     void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (!o || !t || !out || !workspace || planes <= 0 || n_per <= 0 || !aligned8(workspace) || !aligned8(out))
        return BFM_E_ARG;
    if (planes > 65535) return BFM_E_SHAPE;
    if (workspace_bytes < bfm_eval_channel_sums_workspace(planes, n_per)) return BFM_E_WORKSPACE;
    double* part = static_cast<double*>(workspace);
    const int nb = channel_blocks(n_per);
    hipLaunchKernelGGL(channel_sums_kernel, dim3(nb, planes), dim3(NT), 0, bfm_s(stream), o, t, n_per, part);
    hipLaunchKernelGGL(fold_kernel, dim3(planes), dim3(NT), 0, bfm_s(stream), part, nb, 2, 0u, 0u, 1.0, out);
    return bfm_launch_status();
}

extern "C" int bfm_eval_label_counts(const int32_t* P, const int32_t* T, int64_t n, const int32_t* lut, int nlut,
                                     int n_labels, int64_t* counts, bfm_stream_t stream) {
    if (!P || !T || !lut || !counts || n <= 0 || nlut <= 0 || n_labels <= 0 || !aligned8(counts)) return BFM_E_ARG;
    if (n_labels > MAX_LABELS || n > ((int64_t)1 << 40)) return BFM_E_SHAPE;    // a block's 32-bit bins hold its share
    if (hipMemsetAsync(counts, 0, (size_t)(3 * n_labels + 1) * sizeof(int64_t), bfm_s(stream)) != hipSuccess)
        return BFM_E_LAUNCH;
    const int vec = aligned16(P) && aligned16(T);
    hipLaunchKernelGGL(label_counts_kernel, dim3(std::min(LABEL_BLOCKS, stream_blocks(n))), dim3(NT), 0, bfm_s(stream), P, T, n, vec, lut, nlut,
                       n_labels, reinterpret_cast<unsigned long long*>(counts));
    return bfm_launch_status();
}

extern "C" size_t bfm_eval_ssim3d_workspace(int planes, int D, int H, int W) {
    if (planes <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    const SsimPlan p = ssim_plan(planes, D, H, W);
    return (size_t)planes * p.nchunk * p.tiles * 2 * sizeof(double);
}

extern "C" int bfm_eval_ssim3d(const float* X, const float* Y, int planes, int D, int H, int W, const float* win_host,
                               const double* norm_dev, double* out, void* workspace, size_t workspace_bytes,
                               bfm_stream_t stream) {
    if (!X || !Y || !win_host || !out || !workspace || planes <= 0 || D <= 0 || H <= 0 || W <= 0 ||
        !aligned8(workspace) || !aligned8(out) || (norm_dev && !aligned8(norm_dev)))
        return BFM_E_ARG;
    if (planes > 65535 || (int64_t)H * W > INT32_MAX) return BFM_E_SHAPE;
    const SsimPlan p = ssim_plan(planes, D, H, W);
    if (p.nchunk > 65535) return BFM_E_SHAPE;
    if (workspace_bytes < bfm_eval_ssim3d_workspace(planes, D, H, W)) return BFM_E_WORKSPACE;
    SsimWin win;
    for (int k = 0; k < KW; ++k) win.g[k] = win_host[k];
    double* part = static_cast<double*>(workspace);
    const dim3 grid(p.tiles, p.nchunk, planes);
    const int sel = (D >= KW ? 4 : 0) | (H >= KW ? 2 : 0) | (W >= KW ? 1 : 0);
#define BFM_SSIM_LAUNCH(FX, FY, FZ)                                                                                    \
    hipLaunchKernelGGL((ssim3d_kernel<FX, FY, FZ>), grid, dim3(NT), 0, bfm_s(stream), X, Y, D, H, W, p, win, norm_dev, part)
    switch (sel) {
        case 0: BFM_SSIM_LAUNCH(false, false, false); break;
        case 1: BFM_SSIM_LAUNCH(false, false, true); break;
        case 2: BFM_SSIM_LAUNCH(false, true, false); break;
        case 3: BFM_SSIM_LAUNCH(false, true, true); break;
        case 4: BFM_SSIM_LAUNCH(true, false, false); break;
        case 5: BFM_SSIM_LAUNCH(true, false, true); break;
        case 6: BFM_SSIM_LAUNCH(true, true, false); break;
        default: BFM_SSIM_LAUNCH(true, true, true); break;
    }
#undef BFM_SSIM_LAUNCH
    hipLaunchKernelGGL(fold_kernel, dim3(planes), dim3(NT), 0, bfm_s(stream), part, p.nchunk * p.tiles, 2, 0u, 0u,
                       1.0 / ((double)p.Do * (double)p.Ho * (double)p.Wo), out);
    return bfm_launch_status();
}

extern "C" int bfm_eval_avgpool2_pair(const float* X, const float* Y, int planes, int D, int H, int W,
                                      const double* norm_dev, float* Xo, float* Yo, bfm_stream_t stream) {
    if (!X || !Y || !Xo || !Yo || planes <= 0 || D <= 0 || H <= 0 || W <= 0 || (norm_dev && !aligned8(norm_dev)))
        return BFM_E_ARG;
    const int Dp = (D + 1) / 2, Hp = (H + 1) / 2, Wp = (W + 1) / 2;
    const int64_t total = (int64_t)planes * Dp * Hp * Wp;
    hipLaunchKernelGGL(avgpool2_pair_kernel, dim3((unsigned)std::min<int64_t>(8192, bfm_cdiv64(total, NT))), dim3(NT), 0,
                       bfm_s(stream), X, Y, D, H, W, Dp, Hp, Wp, total, norm_dev, Xo, Yo);
    return bfm_launch_status();
}
