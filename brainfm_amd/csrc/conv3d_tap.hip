// The smallest deep-level convolutions as tap-wise GEMMs on densely packed rows.
//
// A 3x3x3 zero-padded conv over nearest_up(y) (y: the GroupNorm-affine-applied low-res tensor of n_lo voxels) is
//      out[o] = sum_tap W[tap] . y[map(o + tap - 1)] = sum_tap P[tap][map(o + tap - 1)],      P[tap][v] = W[tap] . y[v]
// (a term is dropped where o + tap - 1 leaves the hi-res volume).  P is one GEMM per tap with M = S * n_lo rows -- the
// (sample, voxel) pairs of the whole batch packed densely, 64-100 rows at the deepest levels of the 80-wide tiles -- K = Cin
// and N = Cout, instead of S * n_hi rows x 27 taps of which conv_mfma fills 8-50 of every 128-row tile.  With the identity
// map (one source) the same two steps are a plain conv on a tiny volume.  The launch is then what it has to be: one pass
// over the packed weights.
//
//   tap_prep   X [S][n_lo][Cin] fp32 -> affine, * a_scale(sample), split fp16 -> MFMA operand fragments [kc][mb][hi, lo][lane]
//   tap_gemm   workgroup = (Cout tile of 64, tap, K slab) over EVERY row: each weight byte leaves HBM once per launch.  Both
//              operands stream global -> VGPR as whole 1 KB fragments (the weights are conv_mfma's own pack, one tap of one
//              K chunk = a contiguous 4 KB piece), three K chunks in flight per wave.  The four waves take the slab's K
//              chunks round robin and fold their partial sums through LDS in wave order.
//   tap_sum    out[s][o] = (accumulate ? out : 0) + sum_tap sum_slab P[tap][slab][s * n_lo + table[o][tap]], taps and slabs
//              ascending; optional LeakyReLU; optional moment rows in splitk_reduce_rows' form.
//
// Numerics are the family's (conv3d_mfma.hip): hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulate, a_scale
// from the sample's bound.  A row's products and sums do not depend on which rows it is packed with: the K slab plan is a
// function of (Cin, Cout) alone, and rows of an MFMA are independent.
#include "conv_shared.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int KC = 16;
constexpr int TAP_MB = 4;                       // 32-row blocks a workgroup holds accumulators for at a time (128 rows)
constexpr int TAP_THREADS = 256;
constexpr int TAP_LDS = 4 * TAP_MB * 2 * 16 * 64 * (int)sizeof(float);      // the four waves' partial sums: 128 KB

struct TapParams {
    const float* X;
    int Cin, S, n_lo, M, nmbt;       // M = S * n_lo rows in nmbt blocks of 32
    const float *scale, *shift;
    int saff;
    const float* bound;
    int G;
    const uint4* wp;
    int wexp, Cout;
    int kc0, kcn_pack;               // first K chunk of these channels in the pack, K chunks per Cout tile of the pack
    int KCN, kc_per_slab, nslab;
    uint4* apack;                    // [KCN][nmbt][hi, lo][64]
    float* rowdq;                    // [nmbt * 32] 2^-(aexp(sample) + wexp); 0 for padding rows
    float* P;                        // [27][nslab][nmbt * 32][Cout]
};

struct TapLayout {
    int nmbt, nslab, per;
    size_t off_apack, off_P, bytes;
};

// K slabs: only where (Cout tile, tap) alone leaves most of the chip idle.  Of (Cin, Cout) alone, never of the rows.
void tap_split(int Cin, int Cout, int& nslab, int& per) {
    const int KCN = Cin / KC;
    const int wgs = (Cout / 64) * 27;
    nslab = 1;
    per = KCN;
    if (wgs >= 256) return;
    const int want = std::min(std::max(1, KCN / 3), bfm_cdiv(512, wgs));
    if (want < 2) return;
    per = bfm_cdiv(KCN, want);
    nslab = bfm_cdiv(KCN, per);
}

bool tap_layout(int Cin, int Cout, int S, int n_lo, TapLayout& t) {
    if (Cin <= 0 || Cout <= 0 || S <= 0 || n_lo <= 0 || Cin % KC || Cout % 64) return false;
    const int64_t M = (int64_t)S * n_lo;
    if (M > (1 << 20)) return false;
    t.nmbt = (int)bfm_cdiv64(M, 32);
    tap_split(Cin, Cout, t.nslab, t.per);
    const size_t mpad = (size_t)t.nmbt * 32;
    t.off_apack = (mpad * sizeof(float) + 255) / 256 * 256;
    t.off_P = t.off_apack + (size_t)(Cin / KC) * t.nmbt * 2 * 64 * sizeof(uint4);
    t.bytes = t.off_P + (size_t)27 * t.nslab * mpad * Cout * sizeof(float);
    return true;
}

// one 64-thread block = one (K chunk, 32-row block): lane l holds row mb * 32 + (l & 31), channels kc * 16 + 8 (l >> 5) ..
__global__ void __launch_bounds__(64) tap_prep(const TapParams p) {
    const int lane = threadIdx.x;
    const int kc = blockIdx.x, mb = blockIdx.y;
    const int row = mb * 32 + (lane & 31);
    const int k0 = kc * KC + 8 * (lane >> 5);
    half8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) { hi[j] = (_Float16)0.f; lo[j] = (_Float16)0.f; }
    float dq = 0.f;
    if (row < p.M) {
        const int smp = row / p.n_lo;
        const float* pbound = p.bound + (size_t)smp * p.G;
        float bmax = 0.f;
        for (int g = 0; g < p.G; ++g) bmax = fmaxf(bmax, pbound[g]);
        int aexp = 0;
        if (bmax > 0.f && bmax < INFINITY) {
            int ex;
            (void)frexpf(bmax, &ex);
            aexp = 14 - ex;
            aexp = aexp > 60 ? 60 : (aexp < -60 ? -60 : aexp);
        }
        const float a_scale = ldexpf(1.0f, aexp);
        dq = ldexpf(1.0f, -(aexp + p.wexp));
        const float* x = p.X + (size_t)row * p.Cin + k0;
        const float* sc = p.scale + (size_t)smp * p.saff + k0;
        const float* sh = p.shift + (size_t)smp * p.saff + k0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 xv = *reinterpret_cast<const float4*>(x + 4 * q);
            const float4 sv = *reinterpret_cast<const float4*>(sc + 4 * q);
            const float4 hv = *reinterpret_cast<const float4*>(sh + 4 * q);
            const float y[4] = {xv.x, xv.y, xv.z, xv.w};
            const float s4[4] = {sv.x * a_scale, sv.y * a_scale, sv.z * a_scale, sv.w * a_scale};
            const float h4[4] = {hv.x * a_scale, hv.y * a_scale, hv.z * a_scale, hv.w * a_scale};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = fmaf(y[i], s4[i], h4[i]);
                const _Float16 hh = (_Float16)t;
                hi[4 * q + i] = hh;
                lo[4 * q + i] = (_Float16)(t - (float)hh);
            }
        }
    }
    uint4* dst = p.apack + ((size_t)(kc * p.nmbt + mb) * 2) * 64 + lane;
    dst[0] = __builtin_bit_cast(uint4, hi);
    dst[64] = __builtin_bit_cast(uint4, lo);
    if (kc == 0 && lane < 32) p.rowdq[row] = dq;
}

template <int NPASS>
struct TapFrag {
    uint4 w[4];                      // [column block][hi, lo]
    uint4 a[TAP_MB][2];              // [row block][hi, lo]
};

template <int NPASS>
__global__ void __launch_bounds__(TAP_THREADS, 1) tap_gemm(const TapParams p) {
    extern __shared__ __attribute__((aligned(16))) float tap_lds[];       // [wave][(mb * 2 + nb) * 16 + i][lane]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tap = blockIdx.x % 27;
    const int r_ = blockIdx.x / 27;
    const int slab = r_ % p.nslab, nt = r_ / p.nslab;
    const int kcA = slab * p.kc_per_slab, kcB = min(p.KCN, kcA + p.kc_per_slab);
    const uint4* const wb = p.wp + ((size_t)(nt * p.kcn_pack + p.kc0) * 27 + tap) * 256 + lane;     // + kc * 27 * 256
    const int khalf = lane >> 5, l32 = lane & 31;
    const size_t mpad = (size_t)p.nmbt * 32;
    float* const Pt = p.P + ((size_t)(tap * p.nslab + slab) * mpad) * p.Cout + nt * 64 + khalf * 4;

    for (int rg = 0; rg < p.nmbt; rg += TAP_MB) {
        const int nmb = min(TAP_MB, p.nmbt - rg);
        const uint4* const ab = p.apack + (size_t)rg * 128 + lane;                                  // + kc * nmbt * 128
        floatx16 acc[TAP_MB][2];
#pragma unroll
        for (int mb = 0; mb < TAP_MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;

        auto load = [&](int kc, TapFrag<NPASS>& f) __attribute__((always_inline)) {
            if (kc >= kcB) return;
            const uint4* w = wb + (size_t)kc * (27 * 256);
            const uint4* a = ab + (size_t)kc * p.nmbt * 128;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f.w[nb * 2] = w[nb * 128];
                if constexpr (NPASS == 3) f.w[nb * 2 + 1] = w[nb * 128 + 64];
            }
#pragma unroll
            for (int mb = 0; mb < TAP_MB; ++mb)
                if (mb < nmb) {
                    f.a[mb][0] = a[mb * 128];
                    if constexpr (NPASS == 3) f.a[mb][1] = a[mb * 128 + 64];
                }
        };
        auto compute = [&](const TapFrag<NPASS>& f) __attribute__((always_inline)) {
#pragma unroll
            for (int mb = 0; mb < TAP_MB; ++mb)
                if (mb < nmb) {
                    const half8 ahi = __builtin_bit_cast(half8, f.a[mb][0]);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const half8 bhi = __builtin_bit_cast(half8, f.w[nb * 2]);
                        if constexpr (NPASS == 3) {
                            const half8 alo = __builtin_bit_cast(half8, f.a[mb][1]);
                            const half8 blo = __builtin_bit_cast(half8, f.w[nb * 2 + 1]);
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bhi, alo, acc[mb][nb], 0, 0, 0);
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(blo, ahi, acc[mb][nb], 0, 0, 0);
                        }
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bhi, ahi, acc[mb][nb], 0, 0, 0);
                    }
                }
        };

        // this wave's K chunks: kcA + wave, + 4, ...; a ring of three fragment sets, two chunks ahead of the products
        TapFrag<NPASS> f0, f1, f2;
        int kc = kcA + wave;
        load(kc, f0);
        load(kc + 4, f1);
        for (; kc < kcB; kc += 12) {
            load(kc + 8, f2);
            __builtin_amdgcn_sched_barrier(0);           // pin the prefetch: the scheduler would sink it to its first use
            compute(f0);
            if (kc + 4 < kcB) {
                load(kc + 12, f0);
                __builtin_amdgcn_sched_barrier(0);
                compute(f1);
            }
            if (kc + 8 < kcB) {
                load(kc + 16, f1);
                __builtin_amdgcn_sched_barrier(0);
                compute(f2);
            }
        }

        // fold the four waves' partial sums in wave order; wave w then owns row block rg + w
        float* const mine = tap_lds + (size_t)wave * (TAP_MB * 2 * 16 * 64) + lane;
#pragma unroll
        for (int mb = 0; mb < TAP_MB; ++mb)
            if (mb < nmb) {
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) mine[((mb * 2 + nb) * 16 + i) * 64] = acc[mb][nb][i];
            }
        __syncthreads();
        if (wave < nmb) {
            const int row = (rg + wave) * 32 + l32;
            // lane l holds row l & 31 of the block; register i is cout 8 (i >> 2) + 4 (l >> 5) + (i & 3) of the column block
            if (row < p.M) {
                const float dq = p.rowdq[row];
                float* const o = Pt + (size_t)row * p.Cout;
                const float* const src = tap_lds + (size_t)(wave * 2) * 16 * 64 + lane;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float v[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float* s = src + ((nb * 16) + 4 * g + i) * 64;
                            float t = s[0];
#pragma unroll
                            for (int w = 1; w < 4; ++w) t += s[(size_t)w * (TAP_MB * 2 * 16 * 64)];
                            v[i] = t * dq;
                        }
                        *reinterpret_cast<float4*>(o + nb * 32 + g * 8) = make_float4(v[0], v[1], v[2], v[3]);
                    }
            }
        }
        if (rg + TAP_MB < p.nmbt) __syncthreads();       // the next row group writes the same LDS
    }
}

__host__ __device__ inline int tap_cgb(int CG) { return (CG & 63) == 0 ? 64 : ((CG & 31) == 0 ? 32 : 16); }

// output voxels one workgroup of tap_sum folds into one moment row: splitk_reduce_rows' rule (at most 128 rows per sample)
int tap_rows_vpb(int64_t nvox, int Cout) {
    const int CG = Cout / 4, CGB = tap_cgb(CG), NV = 256 / CGB;
    int64_t vpb = std::max<int64_t>((int64_t)NV * 4, bfm_cdiv64(nvox, 128));
    vpb = bfm_cdiv64(vpb, NV) * NV;
    return (int)std::min<int64_t>(vpb, 0x7fffffff);
}

// Workgroup (rb, cz, s): output voxels [rb * vpb, (rb + 1) * vpb) of sample s on CGB column quads; thread (vl, cgl) takes
// every NV-th voxel.  The moment rows fold as in splitk_reduce_rows: fp32 per thread, fp64 across threads in lane order.
__global__ void __launch_bounds__(256) tap_sum(const float* __restrict__ P, int nslab, int64_t mpad, int n_lo,
                                               const int* __restrict__ table, int n_hi, int Cout, int vpb, int nrows,
                                               float slope, int act, int accum, float* __restrict__ out,
                                               double* __restrict__ rsum, double* __restrict__ rsq,
                                               float* __restrict__ rmn, float* __restrict__ rmx) {
    __shared__ float4 lsh[4][256];
    const int CG = Cout >> 2;
    const int CGB = tap_cgb(CG);
    const int NV = 256 / CGB;
    const int tid = threadIdx.x;
    const int cgl = tid % CGB, vl = tid / CGB;
    const int c4 = blockIdx.y * CGB + cgl;
    const int smp = blockIdx.z, rb = blockIdx.x;
    const int v0 = rb * vpb, v1 = min(n_hi, v0 + vpb);
    const float4* P4 = reinterpret_cast<const float4*>(P) + (int64_t)smp * n_lo * CG + c4;
    float4* o4 = reinterpret_cast<float4*>(out);
    float4 fs = make_float4(0.f, 0.f, 0.f, 0.f), fq = fs;
    float4 mn = make_float4(INFINITY, INFINITY, INFINITY, INFINITY), mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int v = v0 + vl; v < v1; v += NV) {
        const int* tb = table + (size_t)v * 27;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 9
        for (int tap = 0; tap < 27; ++tap) {
            const int r = tb[tap];
            if (r < 0 || r >= n_lo) continue;
            for (int k = 0; k < nslab; ++k) {
                const float4 t = P4[((int64_t)(tap * nslab + k) * mpad + r) * CG];
                a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
            }
        }
        const int64_t i = ((int64_t)smp * n_hi + v) * CG + c4;
        if (accum) {
            const float4 t = o4[i];
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        if (act) {
            a.x = a.x >= 0.f ? a.x : a.x * slope; a.y = a.y >= 0.f ? a.y : a.y * slope;
            a.z = a.z >= 0.f ? a.z : a.z * slope; a.w = a.w >= 0.f ? a.w : a.w * slope;
        }
        o4[i] = a;
        fs.x += a.x; fs.y += a.y; fs.z += a.z; fs.w += a.w;
        fq.x = fmaf(a.x, a.x, fq.x); fq.y = fmaf(a.y, a.y, fq.y); fq.z = fmaf(a.z, a.z, fq.z); fq.w = fmaf(a.w, a.w, fq.w);
        mn.x = fminf(mn.x, a.x); mn.y = fminf(mn.y, a.y); mn.z = fminf(mn.z, a.z); mn.w = fminf(mn.w, a.w);
        mx.x = fmaxf(mx.x, a.x); mx.y = fmaxf(mx.y, a.y); mx.z = fmaxf(mx.z, a.z); mx.w = fmaxf(mx.w, a.w);
    }
    if (!rsum) return;                                    // uniform: no moment rows asked for
    lsh[0][tid] = fs; lsh[1][tid] = fq; lsh[2][tid] = mn; lsh[3][tid] = mx;
    __syncthreads();
    if (vl == 0) {
        double S[4] = {0.0, 0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0};
        float MN[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, MX[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int j = 0; j < NV; ++j) {
            const float4 a = lsh[0][j * CGB + cgl], b = lsh[1][j * CGB + cgl], c = lsh[2][j * CGB + cgl], d = lsh[3][j * CGB + cgl];
            S[0] += (double)a.x; S[1] += (double)a.y; S[2] += (double)a.z; S[3] += (double)a.w;
            Q[0] += (double)b.x; Q[1] += (double)b.y; Q[2] += (double)b.z; Q[3] += (double)b.w;
            MN[0] = fminf(MN[0], c.x); MN[1] = fminf(MN[1], c.y); MN[2] = fminf(MN[2], c.z); MN[3] = fminf(MN[3], c.w);
            MX[0] = fmaxf(MX[0], d.x); MX[1] = fmaxf(MX[1], d.y); MX[2] = fmaxf(MX[2], d.z); MX[3] = fmaxf(MX[3], d.w);
        }
        const size_t o = ((size_t)smp * nrows + rb) * Cout + (size_t)c4 * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) { rsum[o + k] = S[k]; rsq[o + k] = Q[k]; rmn[o + k] = MN[k]; rmx[o + k] = MX[k]; }
    }
}

}  // namespace

extern "C" size_t bfm_conv3x3x3_tap_batch_workspace(int Cin, int Cout, int S, int n_lo) {
    TapLayout t;
    return tap_layout(Cin, Cout, S, n_lo, t) ? t.bytes : 0;
}

extern "C" int bfm_conv3x3x3_tap_batch(const float* X, int Cin, int S, int n_lo, const float* scale, const float* shift,
                                       const float* bound, int G, const void* wpacked, int wexp, int Cout, int kc_first,
                                       int kc_pack, int passes, void* workspace, size_t workspace_bytes,
                                       int affine_stride, bfm_stream_t stream) {
    if (!X || !scale || !shift || !bound || G <= 0 || !wpacked || !workspace) return BFM_E_ARG;
    if (passes != 1 && passes != 3) return BFM_E_ARG;
    if (S <= 0 || S > 65535) return BFM_E_ARG;
    TapLayout t;
    if (!tap_layout(Cin, Cout, S, n_lo, t)) return BFM_E_SHAPE;
    if (kc_first < 0 || kc_pack < kc_first + Cin / KC) return BFM_E_ARG;
    if (affine_stride != 0 && (affine_stride < Cin || (affine_stride & 3))) return BFM_E_ARG;
    if (workspace_bytes < t.bytes) return BFM_E_ARG;
    if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(scale) & 15) ||
        (reinterpret_cast<uintptr_t>(shift) & 15) || (reinterpret_cast<uintptr_t>(wpacked) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 255))
        return BFM_E_ARG;
    const int64_t wgs = (int64_t)(Cout / 64) * 27 * t.nslab;
    if (wgs > 0x7fffffff || t.nmbt > 65535) return BFM_E_SHAPE;
    TapParams p{};
    p.X = X; p.Cin = Cin; p.S = S; p.n_lo = n_lo; p.M = S * n_lo; p.nmbt = t.nmbt;
    p.scale = scale; p.shift = shift; p.saff = affine_stride > 0 ? affine_stride : Cin;
    p.bound = bound; p.G = G;
    p.wp = static_cast<const uint4*>(wpacked);
    p.wexp = wexp; p.Cout = Cout; p.kc0 = kc_first; p.kcn_pack = kc_pack;
    p.KCN = Cin / KC; p.kc_per_slab = t.per; p.nslab = t.nslab;
    char* ws = static_cast<char*>(workspace);
    p.rowdq = reinterpret_cast<float*>(ws);
    p.apack = reinterpret_cast<uint4*>(ws + t.off_apack);
    p.P = reinterpret_cast<float*>(ws + t.off_P);
    static bool attr = false;
    if (const int rc = bfm_raise_lds_limit(attr, {bfm_kernel(&tap_gemm<3>), bfm_kernel(&tap_gemm<1>)}, TAP_LDS)) return rc;
    hipLaunchKernelGGL(tap_prep, dim3((unsigned)p.KCN, (unsigned)t.nmbt), dim3(64), 0, bfm_s(stream), p);
    bfm_launch_by_passes(passes, tap_gemm<3>, tap_gemm<1>, dim3((unsigned)wgs), dim3(TAP_THREADS), (size_t)TAP_LDS,
                         bfm_s(stream), p);
    return bfm_launch_status();
}

extern "C" int bfm_tap_sum_rows(int n_hi, int Cout) {
    if (n_hi <= 0 || Cout <= 0 || Cout % 64) return 0;
    return (int)bfm_cdiv64(n_hi, tap_rows_vpb(n_hi, Cout));
}

extern "C" int bfm_tap_sum_batch(const void* workspace, int Cin, int Cout, int S, int n_lo, const int* table, int n_hi,
                                 float slope, int activation, int accumulate, float* out, void* moment_rows,
                                 bfm_stream_t stream) {
    if (!workspace || !table || !out || n_hi <= 0) return BFM_E_ARG;
    if (S <= 0 || S > 65535) return BFM_E_ARG;
    TapLayout t;
    if (!tap_layout(Cin, Cout, S, n_lo, t)) return BFM_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(out) & 15)) return BFM_E_ARG;
    const int vpb = tap_rows_vpb(n_hi, Cout);
    const int nrows = (int)bfm_cdiv64(n_hi, vpb);
    MomentRows mr;
    if (moment_rows && !mr.carve(moment_rows, (size_t)S * nrows * Cout)) return BFM_E_ARG;
    const int CG = Cout / 4, CGB = tap_cgb(CG);
    const float* P = reinterpret_cast<const float*>(static_cast<const char*>(workspace) + t.off_P);
    hipLaunchKernelGGL(tap_sum, dim3((unsigned)nrows, (unsigned)(CG / CGB), (unsigned)S), dim3(256), 0, bfm_s(stream), P,
                       t.nslab, (int64_t)t.nmbt * 32, n_lo, table, n_hi, Cout, vpb, nrows, slope, activation ? 1 : 0,
                       accumulate ? 1 : 0, out, mr.rsum, mr.rsq, mr.rmn, mr.rmx);
    return bfm_launch_status();
}
