// conv_wino's F(2,3) arithmetic on boxes of 5 x 5 x 10 output voxels, for the batched levels whose volumes are 5, 10 and 20
// voxels wide (an 80-wide tile from level 2 down): no power-of-two box divides them, so conv_wino / conv_wino4d fill a
// third to two thirds of their rows there and the direct family (27 of 27 tap-rows where F(2,3) issues 18) ran them.
//
// A 5 (z) x 5 (y) x 10 (x) box is 125 x-pairs: rows 0..124 of the 128 MFMA rows of every Winograd position, pair
// q = (d * 5 + h) * 5 + j; rows 125..127 multiply pair 124 again and are dropped after the output transform.  The box
// divides the volume exactly (D % 5 == 0, H % 5 == 0, W % 10 == 0, else BFM_E_SHAPE), so no row is ever clipped and a box
// never straddles two samples.  Transforms, the hi*hi + hi*lo + lo*hi split, the operand scale from the GroupNorm bound,
// the zero padding after the affine, the weight ring and the weight pack (bfm_pack_conv_weights_wino) are conv_wino's
// (conv3d_wino.hip); the halo'd box is 7 x 7 x 5 = 245 pair positions per plane, 16 planes = 64.3 KB of LDS at KC = 16,
// 66 KB for the output transform: two workgroups per CU.
//
// These volumes are small -- 20^3 is 32 boxes, 10^3 is 4 -- so the K loop is split: workgroup (box, cout tile, slab) runs
// kc_per 16-channel chunks and leaves its output-transformed, dequantised sums in slab `ks` of a workspace; b5_reduce
// sums the slabs in slab order (no atomics), adds what `out` holds (accumulate mode), applies LeakyReLU, stores and
// writes one moment row per box.  The split factor is a function of the layer's shape alone (b5_splitk), never of S, and
// a sample's workgroups do exactly what they do in a launch of that sample alone.
#include "wino_shared.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int KC = 16;
constexpr int NTHR = 256;
constexpr int MLD = 33;                                  // epilogue LDS row stride in floats (odd: conflict-free)
constexpr int BD = 5, BH = 5, BW = 10;                   // the box
constexpr int PW = BW / 2, HT = BH + 2, ZT = BD + 2;     // pairs per row, halo'd rows per slice, halo'd slices
constexpr int NPOS = ZT * HT * PW;                       // 245 pair positions per plane
constexpr int NPAIR = BD * BH * PW;                      // 125 of the 128 rows
constexpr int NVOX = BD * BH * BW;
constexpr int PLANE = ((NPOS * 16 + 255) / 256) * 256 + 16;   // bytes per plane (conv_wino's rule)
constexpr int MAX_IT = (NPOS * 4 + NTHR - 1) / NTHR;     // staging items per thread
constexpr int EPI_LDS = 4 * 128 * MLD * (int)sizeof(float);

struct B5Params {
    const float* A;
    int CA, S, D, H, W;
    const float *scale, *shift, *bound;
    int saff, G;
    const uint4* wp;
    int wexp, Cout;
    float* ws;                       // [splitk][S][D * H * W][Cout]
    int nTy, nTx, nMtS, nMt, NT, KCN, splitk, kc_per;
    int64_t sA, sO, slab;            // elements: one sample of A, one sample of a slab, one slab
};

// conv_wino's split_store4: x = hi + lo in fp16, hi truncated (x - hi exact in fp32), lo rounded to nearest
typedef __fp16 fp16x2_t __attribute__((ext_vector_type(2)));
template <bool LO>
__device__ __forceinline__ void split_store4(const float (&t)[4], unsigned char* dp) {
    const fp16x2_t h01 = __builtin_amdgcn_cvt_pkrtz(t[0], t[1]);
    const fp16x2_t h23 = __builtin_amdgcn_cvt_pkrtz(t[2], t[3]);
    uint2 hv;
    hv.x = __builtin_bit_cast(unsigned, h01);
    hv.y = __builtin_bit_cast(unsigned, h23);
    *reinterpret_cast<uint2*>(dp) = hv;
    if constexpr (LO) {
        uint2 lv;
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lv.x) : "v"(hv.x), "v"(t[0]));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lv.x) : "v"(hv.x), "v"(t[1]));
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lv.y) : "v"(hv.y), "v"(t[2]));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lv.y) : "v"(hv.y), "v"(t[3]));
        *reinterpret_cast<uint2*>(dp + PLANE) = lv;
    }
}

// Workgroup = 4 waves = the 4 Winograd positions of one box x 64 couts x one K slab; LDS [pos][k-half][hi|lo][position]
// [8 ch] as in conv_wino.  Lane l of a 32-row block reads row l (consecutive pairs are consecutive 16-byte positions inside
// a slice of the box, so the ds_read_b128 lane groups meet no bank twice; no row permutation to undo afterwards).
template <int NPASS>
__global__ void __launch_bounds__(NTHR, 2) conv_wino_b5(const B5Params p) {
    constexpr int NPL = (NPASS == 3) ? 2 : 1;
    constexpr int NF = 2 * NPL;
    constexpr int BATCH = (NPASS == 3) ? 1 : 2;      // staging items loaded together (register budget: 128 accumulators)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    // grid: the boxes of all samples fastest, then cout tiles, then slabs -- the workgroups resident at one time read the
    // same few (cout tile, slab) weight streams
    const int bid = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int pos = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave = Winograd position 0..3
    const int l32 = lane & 31, khalf = lane >> 5;
    const int mt = bid % p.nMt;
    const int rest = bid / p.nMt;
    const int nt = rest % p.NT, ks = rest / p.NT;
    const int smp = mt / p.nMtS, box = mt - smp * p.nMtS;
    const int tx = box % p.nTx;
    const int ty = (box / p.nTx) % p.nTy;
    const int tz = box / (p.nTx * p.nTy);
    const int z0 = tz * BD, y0 = ty * BH, x0 = tx * BW;
    const float* const Ab = p.A + (int64_t)smp * p.sA;
    const float* const scale = p.scale + (int64_t)smp * p.saff;
    const float* const shift = p.shift + (int64_t)smp * p.saff;
    const float* const bound = p.bound + (int64_t)smp * p.G;

    float bmax = 0.f;
    for (int g = 0; g < p.G; ++g) bmax = fmaxf(bmax, bound[g]);
    int aexp = 0;
    if (bmax > 0.f && bmax < INFINITY) {
        int ex;
        (void)frexpf(bmax, &ex);
        aexp = 13 - ex;                                            // |V| <= 2 * bound
        aexp = aexp > 60 ? 60 : (aexp < -60 ? -60 : aexp);
    }
    const float a_scale = ldexpf(1.0f, aexp);
    const float dq = ldexpf(1.0f, -(aexp + p.wexp));

    // A base offsets of the four 32-row blocks: pair (d,h,j), tap (kd,kh) = (0,0) reads halo row (d, h), pair j
    int a_off[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        int q = mb * 32 + l32;
        q = q < NPAIR ? q : NPAIR - 1;                             // rows 125..127: pair 124 again, dropped below
        const int d = q / (BH * PW), r = q - d * (BH * PW), h = r / PW, j = r - h * PW;
        a_off[mb] = ((pos * 2 + khalf) * NPL) * PLANE + ((d * HT + h) * PW + j) * 16;
    }

    // staging items: e = tid + it * NTHR -> (halo row, pair, channel quad); off0 = element offset of voxel
    // (gz, gy, x0 + 2j - 1) channel 0 (may point outside the row: the mask says which of the 4 x positions exist)
    const int q4 = tid & 3;
    int off0[MAX_IT];
    int msk[MAX_IT];                                               // bit i: x position i inside the volume; -1: no item
#pragma unroll
    for (int it = 0; it < MAX_IT; ++it) {
        const int e = tid + it * NTHR;
        off0[it] = 0;
        msk[it] = -1;
        if (e < NPOS * 4) {
            const int ps = e >> 2;
            const int r = ps / PW, j = ps - r * PW;
            const int hz = r / HT, hy = r - hz * HT;
            const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + 2 * j - 1;
            int m = 0;
            if (gz >= 0 && gz < p.D && gy >= 0 && gy < p.H) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (gx + i >= 0 && gx + i < p.W) m |= 1 << i;
            }
            msk[it] = m;
            off0[it] = ((gz * p.H + gy) * p.W + gx) * p.CA;
        }
    }
    const int st_plane = ((q4 >> 1) * NPL) * PLANE + (q4 & 1) * 8;

    floatx16 acc[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;

    // this wave's weight stream (conv_wino's pack): KCN * 9 steps, chunk-major, NF fragments of 64 x uint4 per step; ring of
    // three register sets, two steps ahead (9 % 3 == 0: the set index is the tap index mod 3).  This slab's chunks only.
    const int kc0 = ks * p.kc_per;
    const int kc1 = min(p.KCN, kc0 + p.kc_per);
    const int SN = p.KCN * 9;
    const uint4* wbase = p.wp + (size_t)(nt * 4 + pos) * SN * (NF * 64) + lane;
    uint4 wq[3][NF];
    auto fetch = [&](int s, uint4 (&dst)[NF]) __attribute__((always_inline)) {
        const int sc = s < SN ? s : SN - 1;
#pragma unroll
        for (int f = 0; f < NF; ++f) dst[f] = wbase[(size_t)sc * (NF * 64) + f * 64];
    };
    fetch(kc0 * 9, wq[0]);
    fetch(kc0 * 9 + 1, wq[1]);

    for (int kc = kc0; kc < kc1; ++kc) {
        const int c0 = kc * KC;
        const float* src = Ab + c0 + q4 * 4;
        const float4 sc4 = *reinterpret_cast<const float4*>(scale + c0 + q4 * 4);
        const float4 sh4 = *reinterpret_cast<const float4*>(shift + c0 + q4 * 4);
        const float sc[4] = {sc4.x * a_scale, sc4.y * a_scale, sc4.z * a_scale, sc4.w * a_scale};
        const float sh[4] = {sh4.x * a_scale, sh4.y * a_scale, sh4.z * a_scale, sh4.w * a_scale};
        __syncthreads();                                 // previous chunk's readers are done
#pragma unroll
        for (int b0 = 0; b0 < MAX_IT; b0 += BATCH) {
            float4 v[BATCH][4];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int it = b0 + u;
                if (it >= MAX_IT) break;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[u][i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (msk[it] >= 0 && (msk[it] & (1 << i)))
                        v[u][i] = *reinterpret_cast<const float4*>(src + off0[it] + i * p.CA);
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int it = b0 + u;
                if (it >= MAX_IT) break;
                if (msk[it] < 0) continue;
                float dd[4][4];                          // [x position][channel]: affine, zero padding after it
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = msk[it] & (1 << i);
                    const float y[4] = {v[u][i].x, v[u][i].y, v[u][i].z, v[u][i].w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) dd[i][c] = ok ? fmaf(y[c], sc[c], sh[c]) : 0.f;
                }
                const int e = tid + it * NTHR;
                unsigned char* dst = lds + st_plane + (e >> 2) * 16;
#pragma unroll
                for (int ps = 0; ps < 4; ++ps) {
                    float t[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        t[c] = ps == 0 ? dd[0][c] - dd[2][c]
                             : ps == 1 ? dd[1][c] + dd[2][c]
                             : ps == 2 ? dd[2][c] - dd[1][c]
                                       : dd[1][c] - dd[3][c];
                    split_store4<NPASS == 3>(t, dst + (ps * 2 * NPL) * PLANE);
                }
            }
            __builtin_amdgcn_sched_barrier(0);           // keep the next batch's loads from being hoisted (registers)
        }
        __syncthreads();

#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int s = kc * 9 + t;
            const int kd = t / 3, kh = t - kd * 3;
            const int toff = (kd * HT + kh) * PW * 16;
            const int cur = t % 3;
            uint4 bw[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) bw[f] = wq[cur][f];
            fetch(s + 2, wq[(cur + 2) % 3]);             // issued here and pinned: see conv_wino
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                half8 a[NPL];
#pragma unroll
                for (int hl = 0; hl < NPL; ++hl)
                    a[hl] = *reinterpret_cast<const half8*>(lds + a_off[mb] + hl * PLANE + toff);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const half8 bhi = __builtin_bit_cast(half8, bw[nb * NPL]);
                    if constexpr (NPASS == 3) {
                        const half8 blo = __builtin_bit_cast(half8, bw[nb * NPL + 1]);
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], bhi, acc[mb][nb], 0, 0, 0);
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], blo, acc[mb][nb], 0, 0, 0);
                    }
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], bhi, acc[mb][nb], 0, 0, 0);
                }
            }
        }
    }

    // ================= epilogue: output transform through LDS, into this slab =================
    float* m = reinterpret_cast<float*>(lds);                      // [4 positions][128 accumulator rows][MLD]
    float* mw = m + (pos * 128 + khalf * 4) * MLD + l32;           // this lane's write base
    const int col = tid & 31, row0 = tid >> 5;
    float* const wsb = p.ws + (int64_t)ks * p.slab + (int64_t)smp * p.sO + nt * 64 + col;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        __syncthreads();                                           // A planes (or the previous round) fully consumed
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                mw[(mb * 32 + (i >> 2) * 8 + (i & 3)) * MLD] = acc[mb][nb][i];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int q = row0 + 8 * it;
            if (q >= NPAIR) continue;                              // the padding rows end here
            const int d = q / (BH * PW), r = q - d * (BH * PW), h = r / PW, j = r - h * PW;
            const float m0 = m[(0 * 128 + q) * MLD + col], m1 = m[(1 * 128 + q) * MLD + col];
            const float m2 = m[(2 * 128 + q) * MLD + col], m3 = m[(3 * 128 + q) * MLD + col];
            float* o = wsb + (((int64_t)(z0 + d) * p.H + (y0 + h)) * p.W + x0 + 2 * j) * p.Cout + nb * 32;
            o[0] = ((m0 + m1) + m2) * dq;
            o[p.Cout] = ((m1 - m2) - m3) * dq;
        }
    }
}

// column quads per workgroup of b5_reduce: 64 couts, so that even one 10^3 sample (4 boxes) gives Cout / 16 workgroups
constexpr int RCG = 16, RNV = 256 / RCG;

// Workgroup (box, 64-cout block, sample): sums the slabs of the box's 250 voxels in slab order, adds what `out` holds
// (accum), LeakyReLU, store; thread (vl, cgl) takes every RNV-th voxel of the box on one column quad.  The box's moment
// row folds as in splitk_reduce_rows: fp32 per thread, fp64 across the voxel lanes in lane order.  Row smp * nMtS + box.
__global__ void __launch_bounds__(256) b5_reduce(const float* __restrict__ ws, int splitk, int64_t slab4, int nMtS, int nTy,
                                                 int nTx, int D, int H, int W, int Cout, float slope, int accum,
                                                 float* __restrict__ out, double* __restrict__ rsum,
                                                 double* __restrict__ rsq, float* __restrict__ rmn,
                                                 float* __restrict__ rmx) {
    __shared__ float4 lsh[4][256];
    const int CG = Cout >> 2;
    const int tid = threadIdx.x;
    const int cgl = tid % RCG, vl = tid / RCG;
    const int c4 = blockIdx.y * RCG + cgl;
    const int smp = blockIdx.z, box = blockIdx.x;
    const int tx = box % nTx, ty = (box / nTx) % nTy, tz = box / (nTx * nTy);
    const int z0 = tz * BD, y0 = ty * BH, x0 = tx * BW;
    const int64_t nvox = (int64_t)D * H * W;
    const float4* w4 = reinterpret_cast<const float4*>(ws);
    float4* o4 = reinterpret_cast<float4*>(out);
    float4 fs = make_float4(0.f, 0.f, 0.f, 0.f), fq = fs;
    float4 mn = make_float4(INFINITY, INFINITY, INFINITY, INFINITY), mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll 2
    for (int v = vl; v < NVOX; v += RNV) {
        const int d = v / (BH * BW), r = v - d * (BH * BW), h = r / BW, w = r - h * BW;
        const int64_t vox = ((int64_t)(z0 + d) * H + (y0 + h)) * W + x0 + w;
        const int64_t i = ((int64_t)smp * nvox + vox) * CG + c4;
        float4 a = w4[i];
        for (int k = 1; k < splitk; ++k) {
            const float4 t = w4[i + k * slab4];
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        if (accum) {
            const float4 t = o4[i];
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        a.x = a.x >= 0.f ? a.x : a.x * slope; a.y = a.y >= 0.f ? a.y : a.y * slope;
        a.z = a.z >= 0.f ? a.z : a.z * slope; a.w = a.w >= 0.f ? a.w : a.w * slope;
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
        for (int j = 0; j < RNV; ++j) {
            const float4 a = lsh[0][j * RCG + cgl], b = lsh[1][j * RCG + cgl], c = lsh[2][j * RCG + cgl], e = lsh[3][j * RCG + cgl];
            S[0] += (double)a.x; S[1] += (double)a.y; S[2] += (double)a.z; S[3] += (double)a.w;
            Q[0] += (double)b.x; Q[1] += (double)b.y; Q[2] += (double)b.z; Q[3] += (double)b.w;
            MN[0] = fminf(MN[0], c.x); MN[1] = fminf(MN[1], c.y); MN[2] = fminf(MN[2], c.z); MN[3] = fminf(MN[3], c.w);
            MX[0] = fmaxf(MX[0], e.x); MX[1] = fmaxf(MX[1], e.y); MX[2] = fmaxf(MX[2], e.z); MX[3] = fmaxf(MX[3], e.w);
        }
        const size_t o = ((size_t)smp * nMtS + box) * Cout + (size_t)c4 * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) { rsum[o + k] = S[k]; rsq[o + k] = Q[k]; rmn[o + k] = MN[k]; rmx[o + k] = MX[k]; }
    }
}

bool b5_divides(int D, int H, int W) { return D > 0 && H > 0 && W > 0 && D % BD == 0 && H % BH == 0 && W % BW == 0; }

// K slabs of a layer: enough workgroups from ONE sample to put two on each of the 256 CUs, but no slab shorter than four
// chunks once the layer has sixteen (a slab's prologue and its pass through the workspace must stay small beside its
// products).  Of the layer's shape alone.
int b5_splitk(int CA, int Cout, int D, int H, int W) {
    const int KCN = CA / KC;
    const int wgs = (D / BD) * (H / BH) * (W / BW) * (Cout / 64);
    const int want = bfm_cdiv(512, wgs);
    const int per = std::max(KCN >= 16 ? 4 : 1, bfm_cdiv(KCN, want));
    return bfm_cdiv(KCN, per);
}

}  // namespace

// rows of the output-moment table per sample (one per box), 0 where the box does not divide the volume
extern "C" int bfm_conv3x3x3_wino_b5_rows(int D, int H, int W, int passes) {
    (void)passes;
    if (!b5_divides(D, H, W)) return 0;
    const int64_t n = (int64_t)(D / BD) * (H / BH) * (W / BW);
    return n > 0x7fffffff ? 0 : (int)n;
}

// the K split of a layer shape (1 = none); 0 where the kernel does not take the shape
extern "C" int bfm_conv3x3x3_wino_b5_splitk(int Cin, int Cout, int D, int H, int W) {
    if (Cin <= 0 || Cout <= 0 || Cin % KC || Cout % 64 || !b5_divides(D, H, W)) return 0;
    if ((int64_t)(D / BD) * (H / BH) * (W / BW) * (Cout / 64) > 0x7fffffff) return 0;
    return b5_splitk(Cin, Cout, D, H, W);
}

extern "C" size_t bfm_conv3x3x3_wino_b5_workspace(int Cin, int Cout, int S, int D, int H, int W) {
    const int k = bfm_conv3x3x3_wino_b5_splitk(Cin, Cout, D, H, W);
    if (k <= 0 || S < 1) return 0;
    return (size_t)k * S * D * H * W * Cout * sizeof(float);
}

extern "C" int bfm_conv3x3x3_wino_b5_batch(const float* A, int CA, int S, int D, int H, int W, const float* scale,
                                           const float* shift, const float* bound, int G, const void* wpacked, int wexp,
                                           int Cout, float slope, int passes, int flags, float* out, void* moment_rows,
                                           int affine_stride, void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (S < 1 || S > 65535) return BFM_E_ARG;
    const WinoLaunch a{A, CA, D, H, W, scale, shift, bound, G, wpacked, wexp, Cout, slope, passes, flags, out, moment_rows, stream};
    if (const int rc = bfm_wino_check(a, KC)) return rc;
    if (!b5_divides(D, H, W)) return BFM_E_SHAPE;
    if (affine_stride != 0 && (affine_stride < CA || (affine_stride & 3))) return BFM_E_ARG;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return BFM_E_ARG;
    B5Params p{};
    p.A = A; p.CA = CA; p.S = S; p.D = D; p.H = H; p.W = W;
    p.scale = scale; p.shift = shift; p.bound = bound; p.G = G;
    p.saff = affine_stride > 0 ? affine_stride : CA;
    p.wp = static_cast<const uint4*>(wpacked);
    p.wexp = wexp; p.Cout = Cout;
    p.ws = static_cast<float*>(workspace);
    p.nTy = H / BH; p.nTx = W / BW;
    const int64_t boxes = (int64_t)(D / BD) * p.nTy * p.nTx;
    p.NT = Cout / 64;
    p.KCN = CA / KC;
    if (boxes * p.NT > 0x7fffffff) return BFM_E_SHAPE;
    p.splitk = b5_splitk(CA, Cout, D, H, W);
    p.kc_per = bfm_cdiv(p.KCN, p.splitk);
    if (boxes * S * p.NT * p.splitk > 0x7fffffff) return BFM_E_SHAPE;
    p.nMtS = (int)boxes;
    p.nMt = S * p.nMtS;
    const int64_t nvox = (int64_t)D * H * W;
    p.sA = nvox * CA;
    p.sO = nvox * Cout;
    p.slab = (int64_t)S * p.sO;
    if (workspace_bytes < (size_t)p.splitk * (size_t)p.slab * sizeof(float)) return BFM_E_WORKSPACE;
    MomentRows rows;
    if (moment_rows && !rows.carve(moment_rows, (size_t)p.nMt * Cout)) return BFM_E_ARG;
    const size_t smem = std::max<size_t>((size_t)8 * (passes == 3 ? 2 : 1) * PLANE, (size_t)EPI_LDS);
    static bool attr = false;
    if (const int rc = bfm_raise_lds_limit(attr, {bfm_kernel(&conv_wino_b5<3>), bfm_kernel(&conv_wino_b5<1>)}, EPI_LDS)) return rc;
    hipStream_t st = bfm_s(stream);
    bfm_launch_by_passes(passes, conv_wino_b5<3>, conv_wino_b5<1>, dim3((unsigned)(p.nMt * p.NT * p.splitk)), dim3(NTHR), smem,
                         st, p);
    hipLaunchKernelGGL(b5_reduce, dim3((unsigned)p.nMtS, (unsigned)(Cout / (4 * RCG)), (unsigned)S), dim3(256), 0, st,
                       static_cast<const float*>(workspace), p.splitk, p.slab / 4, p.nMtS, p.nTy, p.nTx, D, H, W, Cout, slope,
                       flags & 1, out, rows.rsum, rows.rsq, rows.rmn, rows.rmx);
    return bfm_launch_status();
}
