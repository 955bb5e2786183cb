// Direct 3x3x3 convolution, exact fp32 FMA, any channel count.
//
// SingleConv 'gcl' body after the statistics: folded GroupNorm affine on load,
// zero padding after the affine, conv (no bias), LeakyReLU
// (Trainer/models/unet3d/buildingblocks.py:31-60).  Used for the Cin=1 stem
// (HBM/L2-bound: K = 27 is not a GEMM) and for widths the MFMA family does not
// take; also serves as the exact-fp32 device reference for the MFMA kernel.
//
// One thread = one output voxel x 8 output channels; blockIdx.y = channel
// group, so the weight addresses are wave-uniform (scalar loads).
#include "conv_shared.h"

namespace {

constexpr int TPB = 256;
constexpr int COT = 8;

__global__ void pack_direct(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ out) {
    // out[tap][ci][co] = w[co][ci][tap]
    int64_t n = (int64_t)27 * Cin * Cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int co = (int)(i % Cout);
        int64_t r = i / Cout;
        int ci = (int)(r % Cin);
        int tap = (int)(r / Cin);
        out[i] = w[((int64_t)co * Cin + ci) * 27 + tap];
    }
}

__global__ void __launch_bounds__(TPB) conv_direct(const float* __restrict__ A, int CA, const float* __restrict__ B,
                                                   int CB, int D, int H, int W, UpView up,
                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                   const float* __restrict__ wp, int Cout, float slope,
                                                   float* __restrict__ out) {
    const int64_t nvox = (int64_t)D * H * W;
    const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int co0 = blockIdx.y * COT;
    const int Cin = CA + CB;
    const bool live = v < nvox;
    const int64_t vv = live ? v : 0;
    const int x = (int)(vv % W);
    const int64_t t = vv / W;
    const int y = (int)(t % H);
    const int z = (int)(t / H);

    float acc[COT];
#pragma unroll
    for (int j = 0; j < COT; ++j) acc[j] = 0.f;

    for (int kd = 0; kd < 3; ++kd) {
        for (int kh = 0; kh < 3; ++kh) {
            for (int kw = 0; kw < 3; ++kw) {
                const int zz = z + kd - 1, yy = y + kh - 1, xx = x + kw - 1;
                const bool inb = live && zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W;
                const int tap = (kd * 3 + kh) * 3 + kw;
                const float* wt = wp + (size_t)tap * Cin * Cout + co0;
                int64_t ia = 0, ib = 0;
                if (inb) {
                    ia = (((int64_t)zz * H + yy) * W + xx) * CA;
                    if (CB > 0) ib = (((int64_t)up.mapD[zz] * up.h + up.mapH[yy]) * up.w + up.mapW[xx]) * CB;
                }
                for (int ci = 0; ci < Cin; ++ci) {
                    float xv = 0.f;
                    if (inb) {
                        float raw = ci < CA ? A[ia + ci] : B[ib + (ci - CA)];
                        xv = fmaf(raw, scale[ci], shift[ci]);
                    }
                    const float* wr = wt + (size_t)ci * Cout;
#pragma unroll
                    for (int j = 0; j < COT; ++j) {
                        float wv = (co0 + j < Cout) ? wr[j] : 0.f;
                        acc[j] = fmaf(xv, wv, acc[j]);
                    }
                }
            }
        }
    }
    if (!live) return;
    float* o = out + v * Cout + co0;
#pragma unroll
    for (int j = 0; j < COT; ++j) {
        if (co0 + j < Cout) {
            float r = acc[j];
            o[j] = r >= 0.f ? r : r * slope;
        }
    }
}

// Cin == 1 stem (enc0.1: 1 -> 32 @ up to 160^3) as a K = 32 GEMM on the matrix core: the 27 taps (+5 zero
// columns) are the K dimension, 32 consecutive voxels of one x-run the rows, Cout the columns.  The layer is
// bound by its 128 B/voxel output; with v_mfma_f32_32x32x16_f16 (hi/lo split like conv_mfma, fp32-grade) the
// arithmetic is ~6 MFMAs per 32 voxels and every store instruction writes two full 128-byte output lines.
typedef _Float16 half8s __attribute__((ext_vector_type(8)));
typedef float floatx16s __attribute__((ext_vector_type(16)));
typedef __fp16 fp16x2s __attribute__((ext_vector_type(2)));

template <int NB>
__global__ void __launch_bounds__(256, 3) conv_stem_mfma(const float* __restrict__ A, int D, int H, int W,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         const float* __restrict__ bound,
                                                         const float* __restrict__ wp /*[27][Cout]*/, float slope,
                                                         float* __restrict__ out, int64_t nblocks32,
                                                         double* __restrict__ rsum, double* __restrict__ rsq,
                                                         float* __restrict__ rmn, float* __restrict__ rmx) {
    constexpr int Cout = NB * 32;
    const int lane = threadIdx.x & 63;
    const int l32 = lane & 31, kh = lane >> 5;
    // operand scales (powers of two): activations from the GroupNorm bound, weights from max|w|
    float bmax = bound[0];
    int aexp = 0;
    if (bmax > 0.f && bmax < INFINITY) { int ex; (void)frexpf(bmax, &ex); aexp = 14 - ex; aexp = aexp > 60 ? 60 : (aexp < -60 ? -60 : aexp); }
    float wmax = 0.f;
    for (int i = lane; i < 27 * Cout; i += 64) wmax = fmaxf(wmax, fabsf(wp[i]));
    wmax = wave_reduce_max(wmax);
    int wexp = 0;
    if (wmax > 0.f && wmax < INFINITY) { int ex; (void)frexpf(wmax, &ex); wexp = 14 - ex; wexp = wexp > 60 ? 60 : (wexp < -60 ? -60 : wexp); }
    const float sa = ldexpf(1.f, aexp), sw = ldexpf(1.f, wexp), dq = ldexpf(1.f, -(aexp + wexp));
    const float sc = scale[0] * sa, sh = shift[0] * sa;
    const float dqs = dq * slope;

    // B fragments: lane holds B[k = 16*ks + 8*kh + j][col = nb*32 + l32], k = tap index (>= 27 -> 0)
    half8s bhi[NB][2], blo[NB][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * ks + 8 * kh + j;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float w = k < 27 ? wp[k * Cout + nb * 32 + l32] * sw : 0.f;
                const _Float16 h = (_Float16)w;
                bhi[nb][ks][j] = h;
                blo[nb][ks][j] = (_Float16)(w - (float)h);
            }
        }

    const int xb = (W + 31) >> 5;                               // 32-voxel row blocks per x-run
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;

    // gather of one row block: raw input values (the GroupNorm affine is applied later, zero padding stays exact).
    // The kernel is bound by its vector instructions (profiles/r03_hbm_kernels.txt), so everything that does not depend
    // on the block is computed once per lane: tap q's element offset from the block's own voxel (toff) and the set of
    // volume faces the tap must stay inside of (need: bit 0/1 z-1/z+1, 2/3 y-1/y+1, 4/5 x-1/x+1, 6 always -- taps >= 27
    // never load, 7 always -- the lane's own x must be inside the row); per block a tap costs one add, one test, one select.
    int toff[16];
    unsigned need[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int k = 16 * (q >> 3) + (q & 7) + (kh ? 8 : 0);
        const int dz = k / 9 - 1, dy = (k % 9) / 3 - 1, dx = k % 3 - 1;
        toff[q] = k < 27 ? (dz * H + dy) * W + dx : 0;
        unsigned n = 0x80u;
        if (dz < 0) n |= 1u; if (dz > 0) n |= 2u;
        if (dy < 0) n |= 4u; if (dy > 0) n |= 8u;
        if (dx < 0) n |= 16u; if (dx > 0) n |= 32u;
        if (k >= 27) n |= 64u;
        need[q] = n;
    }
    auto gather = [&](int bx, int y, int z, float (&raw)[16], unsigned& mask) __attribute__((always_inline)) {
        const int x = bx * 32 + l32;
        const int base = (z * H + y) * W + x;                      // the launcher keeps D*H*W below 2^31
        // faces this voxel's neighbours would cross (bit set = that neighbour does not exist)
        const unsigned bad = (z == 0 ? 1u : 0u) | (z == D - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == H - 1 ? 8u : 0u) |
                             (x == 0 ? 16u : 0u) | (x >= W - 1 ? 32u : 0u) | 64u | (x >= W ? 0x80u : 0u);
        mask = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const bool inb = (need[q] & bad) == 0;
            raw[q] = A[inb ? base + toff[q] : 0];                  // a tap outside reads element 0 and is masked below
            mask |= inb ? (1u << q) : 0u;
        }
    };

    // optional moment rows of the output: one row per wave ([gridDim.x*4][Cout]), see conv3d_mfma.hip.  Per block the
    // <= 16 values a lane stores per column go through fp32 partials (as conv_mfma's epilogue does with <= 32), then fp64.
    double ms[NB], mq[NB];
    float mmn[NB], mmx[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { ms[nb] = 0.0; mq[nb] = 0.0; mmn[nb] = INFINITY; mmx[nb] = -INFINITY; }

    // block -> (x block, y, z): divided once, then stepped by the (constant) stride in mixed radix
    const int s_bx = (int)(nw % xb), s_y = (int)((nw / xb) % H), s_z = (int)((nw / xb) / H);
    int nbx = (int)(gw % xb), ny = (int)((gw / xb) % H), nz = (int)((gw / xb) / H);
    auto advance = [&]() __attribute__((always_inline)) {
        nbx += s_bx;
        int c = nbx >= xb ? 1 : 0;
        nbx -= c ? xb : 0;
        ny += s_y + c;
        c = ny >= H ? 1 : 0;
        ny -= c ? H : 0;
        nz += s_z + c;
    };
    float raw[16];
    unsigned mask = 0;
    if (gw < nblocks32) gather(nbx, ny, nz, raw, mask);
    for (int64_t blk = gw; blk < nblocks32; blk += nw) {
        const int bx = nbx;
        const int64_t t = (int64_t)nz * H + ny;
        advance();
        float nraw[16];
        unsigned nmask = 0;
        if (blk + nw < nblocks32) gather(nbx, ny, nz, nraw, nmask);    // in flight while this block is multiplied / stored
        // x = hi + lo by truncation, two values per instruction (v_cvt_pkrtz: x - hi is exact in fp32), as conv3d_wino.hip
        half8s ahi[2], alo[2];
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = (mask >> q) & 1u ? fmaf(raw[q], sc, sh) : 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            unsigned hw[4], lw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v0 = v[8 * ks + 2 * j], v1 = v[8 * ks + 2 * j + 1];
                const fp16x2s h = __builtin_amdgcn_cvt_pkrtz(v0, v1);
                const fp16x2s l = __builtin_amdgcn_cvt_pkrtz(v0 - (float)h[0], v1 - (float)h[1]);
                hw[j] = __builtin_bit_cast(unsigned, h);
                lw[j] = __builtin_bit_cast(unsigned, l);
            }
            ahi[ks] = __builtin_bit_cast(half8s, make_uint4(hw[0], hw[1], hw[2], hw[3]));
            alo[ks] = __builtin_bit_cast(half8s, make_uint4(lw[0], lw[1], lw[2], lw[3]));
        }
        float* orow = out + (t * W + bx * 32) * Cout;               // t = z*H + y
        const bool whole = bx * 32 + 32 <= W;                       // wave-uniform: no per-row test on a full block
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            floatx16s acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo[ks], bhi[nb][ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ks], blo[nb][ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ks], bhi[nb][ks], acc, 0, 0, 0);
            }
            float fs = 0.f, fq = 0.f;
            auto emit = [&](bool check) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int rr = (i & 3) + 8 * (i >> 2) + 4 * kh;     // C/D row of this register
                    if (!check || bx * 32 + rr < W) {
                        // LeakyReLU and the dequantisation in one multiply: dq is a power of two, so
                        // acc * (dq * slope) rounds as (acc * dq) * slope does
                        const float r = acc[i] * (acc[i] >= 0.f ? dq : dqs);
                        orow[rr * Cout + nb * 32 + l32] = r;
                        if (rsum) {
                            fs += r; fq = fmaf(r, r, fq);
                            mmn[nb] = fminf(mmn[nb], r); mmx[nb] = fmaxf(mmx[nb], r);
                        }
                    }
                }
            };
            if (whole) emit(false); else emit(true);
            if (rsum) { ms[nb] += (double)fs; mq[nb] += (double)fq; }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) raw[q] = nraw[q];
        mask = nmask;
    }
    if (rsum) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            ms[nb] += __shfl_xor(ms[nb], 32);
            mq[nb] += __shfl_xor(mq[nb], 32);
            mmn[nb] = fminf(mmn[nb], __shfl_xor(mmn[nb], 32));
            mmx[nb] = fmaxf(mmx[nb], __shfl_xor(mmx[nb], 32));
            if (kh == 0) {
                const size_t o = (size_t)gw * Cout + nb * 32 + l32;
                rsum[o] = ms[nb]; rsq[o] = mq[nb]; rmn[o] = mmn[nb]; rmx[o] = mmx[nb];
            }
        }
    }
}

// The stem for a 2-, 3- or 4-channel input (the conditioned / two-stage networks: image + pathology probability, image +
// flipped image + mask; Trainer/models/__init__.py:423-463): the same GEMM with K = 27 * CIN (+ zero columns up to a
// multiple of 16: 64 / 96 / 112), input channels-last [D][H][W][CIN], one scale/shift per channel of the folded
// GroupNorm(1, CIN), one `bound` for all channels.  Split-fp16 operands, three MFMAs per k-step and the epilogue are those of
// conv_stem_mfma (a kernel of its own, so that the CIN == 1 code stays what it was).
//
// K order.  A lane's 8 k-values of a k-step are whole taps where CIN divides 8: slot s of k-step ks in lane half kh is tap
// SPK * (2 ks + kh) + s (SPK = 4 slots of 2 channels, or 2 slots of 4), one 8- or 16-byte load each.  CIN == 3 puts taps
// 0..23 into two 3-channel slots per lane and k-step (j = 0..5) and the 9 values of taps 24..26 into the spare j = 6, 7 of
// the first five (k-step, half) groups.  stem_kmap is that order for the B fragments; the gather below follows it.
//
// Registers: B stays in VGPRs (CIN = 4, Cout = 64: 7 k-steps x 2 x 2 x 4 = 112) and the kernel asks for 2 waves per SIMD
// instead of 3; there is no second gather in flight (the next block's 56 raw values would not fit beside B).
template <int CIN>
__device__ __forceinline__ bool stem_kmap(int ks, int kh, int j, int& tap, int& ci) {
    const int g = 2 * ks + kh;
    if (CIN == 3) {
        if (j < 6) { tap = 2 * g + j / 3; ci = j % 3; return true; }
        const int s = 2 * g + (j - 6);
        tap = 24 + s / 3; ci = s % 3;
        return s < 9;
    }
    tap = (8 / CIN) * g + j / CIN; ci = j % CIN;
    return tap < 27;
}

template <int NB, int CIN>
__global__ void __launch_bounds__(256, 2) conv_stem_mc(const float* __restrict__ A, int D, int H, int W,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ bound,
                                                       const float* __restrict__ wp /*[27][CIN][Cout]*/, float slope,
                                                       float* __restrict__ out, int64_t nblocks32,
                                                       double* __restrict__ rsum, double* __restrict__ rsq,
                                                       float* __restrict__ rmn, float* __restrict__ rmx) {
    static_assert(CIN >= 2 && CIN <= 4, "conv_stem_mfma is the CIN == 1 kernel");
    constexpr int Cout = NB * 32;
    constexpr int KS = (27 * CIN + 15) / 16;                    // k-steps: 4 / 6 / 7
    constexpr int SPK = CIN == 2 ? 4 : 2;                       // whole-tap slots per lane and k-step
    constexpr int NSL = KS * SPK;
    constexpr int NSP = CIN == 3 ? 6 : 1;                       // single values in j = 6, 7 (CIN == 3: k-steps 0..2)
    const int lane = threadIdx.x & 63;
    const int l32 = lane & 31, kh = lane >> 5;
    float bmax = bound[0];
    int aexp = 0;
    if (bmax > 0.f && bmax < INFINITY) { int ex; (void)frexpf(bmax, &ex); aexp = 14 - ex; aexp = aexp > 60 ? 60 : (aexp < -60 ? -60 : aexp); }
    float wmax = 0.f;
    for (int i = lane; i < 27 * CIN * Cout; i += 64) wmax = fmaxf(wmax, fabsf(wp[i]));
    wmax = wave_reduce_max(wmax);
    int wexp = 0;
    if (wmax > 0.f && wmax < INFINITY) { int ex; (void)frexpf(wmax, &ex); wexp = 14 - ex; wexp = wexp > 60 ? 60 : (wexp < -60 ? -60 : wexp); }
    const float sa = ldexpf(1.f, aexp), sw = ldexpf(1.f, wexp), dq = ldexpf(1.f, -(aexp + wexp));
    float sc[CIN], sh[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) { sc[c] = scale[c] * sa; sh[c] = shift[c] * sa; }
    const float dqs = dq * slope;

    // B fragments: lane holds B[k = 16*ks + 8*kh + j][col = nb*32 + l32], k -> (tap, channel) by stem_kmap
    half8s bhi[NB][KS], blo[NB][KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int tap, ci;
            const bool valid = stem_kmap<CIN>(ks, kh, j, tap, ci);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float w = valid ? wp[(tap * CIN + ci) * Cout + nb * 32 + l32] * sw : 0.f;
                const _Float16 h = (_Float16)w;
                bhi[nb][ks][j] = h;
                blo[nb][ks][j] = (_Float16)(w - (float)h);
            }
        }

    const int xb = (W + 31) >> 5;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;

    // per lane, once: the element offset of every slot's tap from the block's own voxel and the faces it must stay inside
    // of (bits as in conv_stem_mfma: 0/1 z-1/z+1, 2/3 y-1/y+1, 4/5 x-1/x+1, 6 no such tap, 7 the lane's own x)
    auto tap_info = [&](int tap, int& off, unsigned& nd) __attribute__((always_inline)) {
        const int dz = tap / 9 - 1, dy = (tap % 9) / 3 - 1, dx = tap % 3 - 1;
        off = tap < 27 ? ((dz * H + dy) * W + dx) * CIN : 0;
        unsigned n = 0x80u;
        if (dz < 0) n |= 1u; if (dz > 0) n |= 2u;
        if (dy < 0) n |= 4u; if (dy > 0) n |= 8u;
        if (dx < 0) n |= 16u; if (dx > 0) n |= 32u;
        if (tap >= 27) n |= 64u;
        nd = n;
    };
    int toff[NSL];
    unsigned need[NSL];
#pragma unroll
    for (int q = 0; q < NSL; ++q) tap_info(SPK * (2 * (q / SPK) + kh) + q % SPK, toff[q], need[q]);
    int soff[NSP];
    unsigned sneed[NSP];
    float ssc[NSP], ssh[NSP];
#pragma unroll
    for (int q = 0; q < NSP; ++q) {
        soff[q] = 0; sneed[q] = 64u; ssc[q] = 0.f; ssh[q] = 0.f;
        if (CIN == 3) {
            int tap, ci;
            const bool valid = stem_kmap<CIN>(q >> 1, kh, 6 + (q & 1), tap, ci);
            tap_info(valid ? tap : 27, soff[q], sneed[q]);
            soff[q] += valid ? ci : 0;
            ssc[q] = ci == 0 ? sc[0] : (ci == 1 ? sc[1] : sc[CIN - 1]);
            ssh[q] = ci == 0 ? sh[0] : (ci == 1 ? sh[1] : sh[CIN - 1]);
        }
    }

    double ms[NB], mq[NB];
    float mmn[NB], mmx[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { ms[nb] = 0.0; mq[nb] = 0.0; mmn[nb] = INFINITY; mmx[nb] = -INFINITY; }

    const int s_bx = (int)(nw % xb), s_y = (int)((nw / xb) % H), s_z = (int)((nw / xb) / H);
    int nbx = (int)(gw % xb), ny = (int)((gw / xb) % H), nz = (int)((gw / xb) / H);
    for (int64_t blk = gw; blk < nblocks32; blk += nw) {
        const int bx = nbx, y = ny, z = nz;
        const int64_t t = (int64_t)z * H + y;
        {
            nbx += s_bx;
            int c = nbx >= xb ? 1 : 0;
            nbx -= c ? xb : 0;
            ny += s_y + c;
            c = ny >= H ? 1 : 0;
            ny -= c ? H : 0;
            nz += s_z + c;
        }
        const int x = bx * 32 + l32;
        const int base = ((z * H + y) * W + x) * CIN;              // the launcher keeps D*H*W*CIN below 2^31
        const unsigned bad = (z == 0 ? 1u : 0u) | (z == D - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == H - 1 ? 8u : 0u) |
                             (x == 0 ? 16u : 0u) | (x >= W - 1 ? 32u : 0u) | 64u | (x >= W ? 0x80u : 0u);
        floatx16s acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            // a slot outside the volume reads element 0 and becomes the exact zero of the padding
            float v[8];
#pragma unroll
            for (int s = 0; s < SPK; ++s) {
                const int q = ks * SPK + s;
                const bool inb = (need[q] & bad) == 0;
                const float* p = A + (inb ? base + toff[q] : 0);
                float r[CIN];
                if constexpr (CIN == 2) { const float2 f = *reinterpret_cast<const float2*>(p); r[0] = f.x; r[1] = f.y; }
                else if constexpr (CIN == 4) { const float4 f = *reinterpret_cast<const float4*>(p); r[0] = f.x; r[1] = f.y; r[2] = f.z; r[3] = f.w; }
                else { r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; }
#pragma unroll
                for (int e = 0; e < CIN; ++e) v[s * CIN + e] = inb ? fmaf(r[e], sc[e], sh[e]) : 0.f;
            }
            if (CIN == 3) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float val = 0.f;
                    if (2 * ks + u < NSP) {
                        const int q = 2 * ks + u;
                        const bool inb = (sneed[q] & bad) == 0;
                        const float raw = A[inb ? base + soff[q] : 0];
                        val = inb ? fmaf(raw, ssc[q], ssh[q]) : 0.f;
                    }
                    v[6 + u] = val;
                }
            }
            // x = hi + lo by truncation, two values per instruction, as conv_stem_mfma
            unsigned hw[4], lw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v0 = v[2 * j], v1 = v[2 * j + 1];
                const fp16x2s h = __builtin_amdgcn_cvt_pkrtz(v0, v1);
                const fp16x2s l = __builtin_amdgcn_cvt_pkrtz(v0 - (float)h[0], v1 - (float)h[1]);
                hw[j] = __builtin_bit_cast(unsigned, h);
                lw[j] = __builtin_bit_cast(unsigned, l);
            }
            const half8s ahi = __builtin_bit_cast(half8s, make_uint4(hw[0], hw[1], hw[2], hw[3]));
            const half8s alo = __builtin_bit_cast(half8s, make_uint4(lw[0], lw[1], lw[2], lw[3]));
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi[nb][ks], acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo[nb][ks], acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi[nb][ks], acc[nb], 0, 0, 0);
            }
        }
        float* orow = out + (t * W + bx * 32) * Cout;               // t = z*H + y
        const bool whole = bx * 32 + 32 <= W;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float fs = 0.f, fq = 0.f;
            auto emit = [&](bool check) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int rr = (i & 3) + 8 * (i >> 2) + 4 * kh;     // C/D row of this register
                    if (!check || bx * 32 + rr < W) {
                        const float r = acc[nb][i] * (acc[nb][i] >= 0.f ? dq : dqs);
                        orow[rr * Cout + nb * 32 + l32] = r;
                        if (rsum) {
                            fs += r; fq = fmaf(r, r, fq);
                            mmn[nb] = fminf(mmn[nb], r); mmx[nb] = fmaxf(mmx[nb], r);
                        }
                    }
                }
            };
            if (whole) emit(false); else emit(true);
            if (rsum) { ms[nb] += (double)fs; mq[nb] += (double)fq; }
        }
    }
    if (rsum) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            ms[nb] += __shfl_xor(ms[nb], 32);
            mq[nb] += __shfl_xor(mq[nb], 32);
            mmn[nb] = fminf(mmn[nb], __shfl_xor(mmn[nb], 32));
            mmx[nb] = fmaxf(mmx[nb], __shfl_xor(mmx[nb], 32));
            if (kh == 0) {
                const size_t o = (size_t)gw * Cout + nb * 32 + l32;
                rsum[o] = ms[nb]; rsq[o] = mq[nb]; rmn[o] = mmn[nb]; rmx[o] = mmx[nb];
            }
        }
    }
}

}  // namespace

extern "C" int bfm_pack_conv_weights_direct(const float* w, int Cin, int Cout, float* wpacked, bfm_stream_t stream) {
    if (!w || !wpacked || Cin <= 0 || Cout <= 0) return BFM_E_ARG;
    int64_t n = (int64_t)27 * Cin * Cout;
    int nb = (int)std::min<int64_t>(2048, bfm_cdiv64(n, 256));
    hipLaunchKernelGGL(pack_direct, dim3(nb), dim3(256), 0, bfm_s(stream), w, Cin, Cout, wpacked);
    return bfm_launch_status();
}

extern "C" int bfm_conv3x3x3_direct(const float* A, int CA, const float* B, int CB, int D, int H, int W,
                                    const bfm_upsample_t* up, const float* scale, const float* shift,
                                    const float* wpacked, int Cout, float slope, float* out, bfm_stream_t stream) {
    if (!A || CA <= 0 || D <= 0 || H <= 0 || W <= 0 || !scale || !shift || !wpacked || Cout <= 0 || !out)
        return BFM_E_ARG;
    if (CB < 0 || (CB > 0 && (!B || !up || !up->mapD || !up->mapH || !up->mapW))) return BFM_E_ARG;
    int64_t nvox = (int64_t)D * H * W;
    dim3 grid((unsigned)bfm_cdiv64(nvox, TPB), (unsigned)bfm_cdiv(Cout, COT));
    hipLaunchKernelGGL(conv_direct, grid, dim3(TPB), 0, bfm_s(stream), A, CA, B, CB, D, H, W, make_upview(up), scale,
                       shift, wpacked, Cout, slope, out);
    return bfm_launch_status();
}

namespace {
int64_t stem_grid(int D, int H, int W) {
    const int64_t nblk = (int64_t)D * H * ((W + 31) / 32);
    int64_t nb = bfm_cdiv64(nblk, 4);
    if (nb > 256 * 16) nb = 256 * 16;
    return nb;
}
}  // namespace

// rows of the output-moment table bfm_conv3x3x3_stem_ex writes (one per wave of the launch)
extern "C" int bfm_conv3x3x3_stem_rows(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return 0;
    return (int)(stem_grid(D, H, W) * 4);
}

extern "C" int bfm_conv3x3x3_stem_ex(const float* A, int D, int H, int W, const float* scale, const float* shift,
                                     const float* bound, const float* wpacked_direct, int Cout, float slope,
                                     float* out, void* moment_rows, bfm_stream_t stream) {
    if (!A || D <= 0 || H <= 0 || W <= 0 || !scale || !shift || !bound || !wpacked_direct || !out) return BFM_E_ARG;
    if (Cout != 32 && Cout != 64) return BFM_E_SHAPE;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return BFM_E_SHAPE;          // the kernel indexes the input with 32 bits
    const int64_t nblk = (int64_t)D * H * ((W + 31) / 32);
    const int64_t nb = stem_grid(D, H, W);
    MomentRows r;
    if (moment_rows && !r.carve(moment_rows, (size_t)nb * 4 * Cout)) return BFM_E_ARG;
    if (Cout == 32)
        hipLaunchKernelGGL(conv_stem_mfma<1>, dim3((unsigned)nb), dim3(256), 0, bfm_s(stream), A, D, H, W, scale, shift,
                           bound, wpacked_direct, slope, out, nblk, r.rsum, r.rsq, r.rmn, r.rmx);
    else
        hipLaunchKernelGGL(conv_stem_mfma<2>, dim3((unsigned)nb), dim3(256), 0, bfm_s(stream), A, D, H, W, scale, shift,
                           bound, wpacked_direct, slope, out, nblk, r.rsum, r.rsq, r.rmn, r.rmx);
    return bfm_launch_status();
}

// Cin in {2, 3, 4}: the stem of a conditioned network (image + condition channels, channels-last).  Same rows as
// bfm_conv3x3x3_stem_rows.  A must be aligned to Cin floats where Cin is 2 or 4 (the kernel loads a voxel at once).
template <int CIN>
static void stem_mc_launch(int Cout, int64_t nb, bfm_stream_t stream, const float* A, int D, int H, int W, const float* scale,
                           const float* shift, const float* bound, const float* wp, float slope, float* out, int64_t nblk,
                           const MomentRows& r) {
    if (Cout == 32)
        hipLaunchKernelGGL((conv_stem_mc<1, CIN>), dim3((unsigned)nb), dim3(256), 0, bfm_s(stream), A, D, H, W, scale, shift,
                           bound, wp, slope, out, nblk, r.rsum, r.rsq, r.rmn, r.rmx);
    else
        hipLaunchKernelGGL((conv_stem_mc<2, CIN>), dim3((unsigned)nb), dim3(256), 0, bfm_s(stream), A, D, H, W, scale, shift,
                           bound, wp, slope, out, nblk, r.rsum, r.rsq, r.rmn, r.rmx);
}

extern "C" int bfm_conv3x3x3_stem_mc_ex(const float* A, int Cin, int D, int H, int W, const float* scale,
                                        const float* shift, const float* bound, const float* wpacked_direct, int Cout,
                                        float slope, float* out, void* moment_rows, bfm_stream_t stream) {
    if (!A || D <= 0 || H <= 0 || W <= 0 || !scale || !shift || !bound || !wpacked_direct || !out) return BFM_E_ARG;
    if (Cin < 2 || Cin > 4) return BFM_E_SHAPE;
    if (Cout != 32 && Cout != 64) return BFM_E_SHAPE;
    if ((int64_t)D * H * W * Cin >= ((int64_t)1 << 31)) return BFM_E_SHAPE;    // the kernel indexes the input with 32 bits
    if (Cin != 3 && (reinterpret_cast<uintptr_t>(A) & (size_t)(4 * Cin - 1))) return BFM_E_ARG;
    const int64_t nblk = (int64_t)D * H * ((W + 31) / 32);
    const int64_t nb = stem_grid(D, H, W);
    MomentRows r;
    if (moment_rows && !r.carve(moment_rows, (size_t)nb * 4 * Cout)) return BFM_E_ARG;
    if (Cin == 2) stem_mc_launch<2>(Cout, nb, stream, A, D, H, W, scale, shift, bound, wpacked_direct, slope, out, nblk, r);
    else if (Cin == 3) stem_mc_launch<3>(Cout, nb, stream, A, D, H, W, scale, shift, bound, wpacked_direct, slope, out, nblk, r);
    else stem_mc_launch<4>(Cout, nb, stream, A, D, H, W, scale, shift, bound, wpacked_direct, slope, out, nblk, r);
    return bfm_launch_status();
}
