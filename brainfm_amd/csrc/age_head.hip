// The pooled scalar (brain-age) head of TaskHead, Trainer/models/head.py:39-48,61-66, forward and backward, fp32:
//
//   feat (D,H,W,C) -> MaxPool3d(4,4) -> Conv3d(C->16,k3,p1,bias) + LeakyReLU(0.2) -> MaxPool3d(4,4)
//        -> Conv3d(16->4,k3,p1,bias) + LeakyReLU(0.2) -> flatten (NCDHW order) -> Linear(N,160)+ReLU -> Linear(160,10)+ReLU
//        -> Linear(10,1)
//
// Every tensor is channels-last; every weight is in torch's own layout (Conv3d (Cout,Cin,3,3,3), Linear (out,in)), so the
// parameters of a reference checkpoint are used as they are.  Plain per-lane FMA (no packed FP32), no
// atomics, every sum in a fixed order: two runs give the same bits.
#include "bfm_common.h"

namespace {

constexpr int NT = 256;
constexpr int H1 = 160;      // final_linear1_age out_features
constexpr int H2 = 10;       // final_linear2_age out_features
constexpr int WCHUNK = 256;  // voxels per partial sum of the convolution weight gradient
constexpr int CPT = 4;       // output channels per thread of the convolution forward

__device__ __forceinline__ float leaky(float s) { return s > 0.f ? s : s * 0.2f; }
__device__ __forceinline__ float relu(float s) { return s < 0.f ? 0.f : s; }

// fixed-order block sum of NT threads: butterfly inside each wave, then the four wave sums in order
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_reduce_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) red[wv] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int k = 0; k < NT / 64; ++k) s += red[k];
    return s;
}

// ---------------------------------------------------------------- MaxPool3d(4, 4), floor mode
// one thread per (window, channel); the window is scanned z, y, x; a later value wins only if it is larger or NaN (the
// rule of nn.MaxPool3d's kernel: first maximum on ties, NaN sticky); arg = dz*16 + dy*4 + dx of the winner
__global__ void __launch_bounds__(NT) maxpool4_kernel(const float* __restrict__ in, int C, int H, int W, int Ph, int Pw,
                                                      float* __restrict__ out, uint8_t* __restrict__ arg, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int px = (int)(p % Pw);
    const int64_t t = p / Pw;
    const int py = (int)(t % Ph), pz = (int)(t / Ph);
    const float* base = in + (((int64_t)(4 * pz) * H + 4 * py) * W + 4 * px) * C + c;
    float v[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) v[k] = base[(((int64_t)(k >> 4) * H + ((k >> 2) & 3)) * W + (k & 3)) * C];
    float best = v[0];
    int bi = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k)
        if (v[k] > best || isnan(v[k])) { best = v[k]; bi = k; }
    out[i] = best;
    arg[i] = (uint8_t)bi;
}

// gradient of the pool, gather form: every element of dst (D,H,W,C) written (its window's gradient at the argmax, 0 elsewhere
// and outside the floor-mode region)
__global__ void __launch_bounds__(NT) maxpool4_bwd_gather_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg,
                                                                 int C, int H, int W, int Pd, int Ph, int Pw,
                                                                 float* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int64_t v = i / C;
    const int x = (int)(v % W);
    const int64_t t = v / W;
    const int y = (int)(t % H), z = (int)(t / H);
    const int pz = z >> 2, py = y >> 2, px = x >> 2;
    float r = 0.f;
    if (pz < Pd && py < Ph && px < Pw) {
        const int64_t j = (((int64_t)pz * Ph + py) * Pw + px) * C + c;
        if ((int)arg[j] == (((z & 3) << 4) | ((y & 3) << 2) | (x & 3))) r = g[j];
    }
    dst[i] = r;
}

// scatter form: dst[argmax] += g, one thread per (window, channel); each target belongs to exactly one window, so a plain
// read-add-write
__global__ void __launch_bounds__(NT) maxpool4_bwd_scatter_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg,
                                                                  int C, int H, int W, int Ph, int Pw,
                                                                  float* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int px = (int)(p % Pw);
    const int64_t t = p / Pw;
    const int py = (int)(t % Ph), pz = (int)(t / Ph);
    const int k = arg[i];
    const int64_t q = ((((int64_t)(4 * pz + (k >> 4))) * H + 4 * py + ((k >> 2) & 3)) * W + 4 * px + (k & 3)) * C + c;
    dst[q] = dst[q] + g[i];
}

// ---------------------------------------------------------------- ConvBlock: Conv3d(k3, s1, p1, bias) + LeakyReLU(0.2)
// one thread per (voxel, CPT output channels)
__global__ void __launch_bounds__(NT) conv_fwd_kernel(const float* __restrict__ x, int Cin, int D, int H, int W,
                                                      const float* __restrict__ w, const float* __restrict__ b, int Cout,
                                                      float* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int ng = Cout / CPT;
    const int g = (int)(i % ng);
    const int64_t v = i / ng;
    const int xx = (int)(v % W);
    const int64_t t = v / W;
    const int yy = (int)(t % H), zz = (int)(t / H);
    float acc[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
    for (int tap = 0; tap < 27; ++tap) {
        const int iz = zz + tap / 9 - 1, iy = yy + (tap / 3) % 3 - 1, ix = xx + tap % 3 - 1;
        if (iz < 0 || iz >= D || iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const float* xp = x + (((int64_t)iz * H + iy) * W + ix) * Cin;
        const float* wp = w + (int64_t)(g * CPT) * Cin * 27 + tap;
        for (int ci = 0; ci < Cin; ++ci) {
            const float xv = xp[ci];
#pragma unroll
            for (int j = 0; j < CPT; ++j) acc[j] += wp[((int64_t)j * Cin + ci) * 27] * xv;
        }
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) y[v * Cout + g * CPT + j] = leaky(acc[j] + b[g * CPT + j]);
}

// gradient at the convolution's output (before the activation): dy * LeakyReLU'(pre); y > 0 exactly where pre > 0
__device__ __forceinline__ float pre_grad(const float* __restrict__ dy, const float* __restrict__ y, int64_t j) {
    const float g = dy[j];
    if (!y) return g;
    return y[j] > 0.f ? g : g * 0.2f;
}

// blocks [0, nb_dgrad): dx, one thread per (voxel, input channel);
// blocks [nb_dgrad, ...): per WCHUNK voxels, the partial weight / bias gradient of one (Cout, Cin + 1) pair per thread (27
// taps each; ci == Cin is the bias)
__global__ void __launch_bounds__(NT) conv_bwd_kernel(const float* __restrict__ x, int Cin, int D, int H, int W,
                                                      const float* __restrict__ w, int Cout, const float* __restrict__ y,
                                                      const float* __restrict__ dy, float* __restrict__ dx, int nb_dgrad,
                                                      int tiles, float* __restrict__ part) {
    const int64_t nvox = (int64_t)D * H * W;
    if ((int)blockIdx.x < nb_dgrad) {
        const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
        if (i >= nvox * Cin) return;
        const int ci = (int)(i % Cin);
        const int64_t v = i / Cin;
        const int xx = (int)(v % W);
        const int64_t t = v / W;
        const int yy = (int)(t % H), zz = (int)(t / H);
        float acc = 0.f;
        for (int tap = 0; tap < 27; ++tap) {
            const int oz = zz - tap / 9 + 1, oy = yy - (tap / 3) % 3 + 1, ox = xx - tap % 3 + 1;
            if (oz < 0 || oz >= D || oy < 0 || oy >= H || ox < 0 || ox >= W) continue;
            const int64_t o = (((int64_t)oz * H + oy) * W + ox) * Cout;
            for (int co = 0; co < Cout; ++co) acc += w[((int64_t)co * Cin + ci) * 27 + tap] * pre_grad(dy, y, o + co);
        }
        dx[i] = acc;
        return;
    }
    const int bb = (int)blockIdx.x - nb_dgrad;
    const int chunk = bb / tiles, tile = bb - chunk * tiles;
    const int P = Cout * (Cin + 1);
    const int idx = tile * NT + (int)threadIdx.x;
    if (idx >= P) return;
    const int co = idx / (Cin + 1), ci = idx - co * (Cin + 1);
    float acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.f;
    const int64_t v0 = (int64_t)chunk * WCHUNK;
    const int64_t v1 = v0 + WCHUNK < nvox ? v0 + WCHUNK : nvox;
    for (int64_t v = v0; v < v1; ++v) {
        const float g = pre_grad(dy, y, v * Cout + co);
        if (ci == Cin) {
            acc[0] += g;
            continue;
        }
        const int xx = (int)(v % W);
        const int64_t t = v / W;
        const int yy = (int)(t % H), zz = (int)(t / H);
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            const int iz = zz + tap / 9 - 1, iy = yy + (tap / 3) % 3 - 1, ix = xx + tap % 3 - 1;
            if (iz < 0 || iz >= D || iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            acc[tap] += g * x[(((int64_t)iz * H + iy) * W + ix) * Cin + ci];
        }
    }
    float* pp = part + ((int64_t)chunk * P + idx) * 27;
#pragma unroll
    for (int k = 0; k < 27; ++k) pp[k] = acc[k];
}

// dw (Cout,Cin,27) and db (Cout): the partials of every chunk added in chunk order
__global__ void __launch_bounds__(NT) conv_wgrad_reduce_kernel(const float* __restrict__ part, int nchunks, int Cin, int Cout,
                                                               float* __restrict__ dw, float* __restrict__ db) {
    const int o = blockIdx.x * NT + threadIdx.x;
    const int nw = Cout * Cin * 27;
    if (o >= nw + Cout) return;
    int idx, tap;
    if (o < nw) {
        const int co = o / (Cin * 27), r = o - co * Cin * 27;
        idx = co * (Cin + 1) + r / 27;
        tap = r % 27;
    } else {
        idx = (o - nw) * (Cin + 1) + Cin;
        tap = 0;
    }
    const int64_t P = (int64_t)Cout * (Cin + 1);
    float s = 0.f;
    for (int k = 0; k < nchunks; ++k) s += part[(k * P + idx) * 27 + tap];
    if (o < nw) dw[o] = s;
    else db[o - nw] = s;
}

// ---------------------------------------------------------------- flatten + the three Linear layers
// flat[i] (NCDHW flatten of the (nv, 4) channels-last conv output): c = i / nv, voxel = i % nv
__global__ void __launch_bounds__(NT) mlp1_kernel(const float* __restrict__ y2, int nv, const float* __restrict__ l1w,
                                                  const float* __restrict__ l1b, int N, float* __restrict__ h1) {
    __shared__ float red[NT / 64];
    const int j = blockIdx.x;
    float acc = 0.f;
    for (int i = threadIdx.x; i < N; i += NT) {
        const int c = i / nv, v = i - c * nv;
        acc += l1w[(int64_t)j * N + i] * y2[v * 4 + c];
    }
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) h1[j] = relu(s + l1b[j]);
}

__global__ void __launch_bounds__(64) mlp23_kernel(const float* __restrict__ h1, const float* __restrict__ l2w,
                                                   const float* __restrict__ l2b, const float* __restrict__ l3w,
                                                   const float* __restrict__ l3b, float* __restrict__ h2, float* __restrict__ out) {
    __shared__ float s2[H2];
    const int k = threadIdx.x;
    if (k < H2) {
        float acc = 0.f;
        for (int j = 0; j < H1; ++j) acc += l2w[k * H1 + j] * h1[j];
        s2[k] = relu(acc + l2b[k]);
        h2[k] = s2[k];
    }
    __syncthreads();
    if (k == 0) {
        float p = 0.f;
        for (int m = 0; m < H2; ++m) p += l3w[m] * s2[m];
        out[0] = p + l3b[0];
    }
}

// loss (criterion.py loss_age: | |p| - age |, float64) and d/dp = coef * sign(|p| - age) * sign(p) -- or dp_in[0] -- then
// the gradients of the two small layers and of final_linear1's pre-activation (-> dpre1)
__global__ void __launch_bounds__(NT) mlp_bwd_small_kernel(const float* __restrict__ h1, const float* __restrict__ h2,
                                                           const float* __restrict__ p, const float* __restrict__ dp_in,
                                                           double age, float coef, double* __restrict__ loss,
                                                           const float* __restrict__ l2w, const float* __restrict__ l3w,
                                                           float* __restrict__ dl1b, float* __restrict__ dl2w,
                                                           float* __restrict__ dl2b, float* __restrict__ dl3w,
                                                           float* __restrict__ dl3b, float* __restrict__ dpre1) {
    __shared__ float s_d2[H2];
    if (threadIdx.x == 0) {
        float dp;
        if (dp_in) {
            dp = dp_in[0];
        } else {
            const double pv = (double)p[0];
            const double diff = fabs(pv) - age;
            if (loss) loss[0] = fabs(diff);
            const float s1 = diff > 0. ? 1.f : (diff < 0. ? -1.f : 0.f);
            const float s2 = pv > 0. ? 1.f : (pv < 0. ? -1.f : 0.f);
            dp = s1 * s2 * coef;
        }
        dl3b[0] = dp;
        for (int k = 0; k < H2; ++k) {
            dl3w[k] = dp * h2[k];
            const float d = h2[k] > 0.f ? dp * l3w[k] : 0.f;
            s_d2[k] = d;
            dl2b[k] = d;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < H1; j += NT) {
        float acc = 0.f;
        for (int k = 0; k < H2; ++k) acc += l2w[k * H1 + j] * s_d2[k];
        const float d = h1[j] > 0.f ? acc : 0.f;
        dpre1[j] = d;
        dl1b[j] = d;
        for (int k = 0; k < H2; ++k) dl2w[k * H1 + j] = s_d2[k] * h1[j];
    }
}

// final_linear1's weight gradient and the gradient at the conv output (flatten undone): one thread per flat index
__global__ void __launch_bounds__(NT) mlp_bwd_l1_kernel(const float* __restrict__ y2, int nv, const float* __restrict__ l1w,
                                                        int N, const float* __restrict__ dpre1, float* __restrict__ dl1w,
                                                        float* __restrict__ dy2) {
    __shared__ float d1[H1];
    for (int j = threadIdx.x; j < H1; j += NT) d1[j] = dpre1[j];
    __syncthreads();
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const int c = i / nv, v = i - c * nv;
    const float fl = y2[v * 4 + c];
    float acc = 0.f;
    for (int j = 0; j < H1; ++j) {
        acc += l1w[(int64_t)j * N + i] * d1[j];
        dl1w[(int64_t)j * N + i] = d1[j] * fl;
    }
    dy2[v * 4 + c] = acc;
}

inline unsigned nblk(int64_t n) { return (unsigned)bfm_cdiv64(n, NT); }

inline int64_t conv_bwd_chunks(int D, int H, int W) { return bfm_cdiv64((int64_t)D * H * W, WCHUNK); }

}  // namespace

extern "C" {

int bfm_maxpool4(const float* in, int C, int D, int H, int W, float* out, uint8_t* arg, bfm_stream_t stream) {
    if (!in || !out || !arg || C <= 0 || D < 4 || H < 4 || W < 4) return BFM_E_ARG;
    const int Pd = D / 4, Ph = H / 4, Pw = W / 4;
    const int64_t n = (int64_t)Pd * Ph * Pw * C;
    hipLaunchKernelGGL(maxpool4_kernel, dim3(nblk(n)), dim3(NT), 0, bfm_s(stream), in, C, H, W, Ph, Pw, out, arg, n);
    return bfm_launch_status();
}

int bfm_maxpool4_bwd(const float* g, const uint8_t* arg, int C, int D, int H, int W, float* dst, int accumulate,
                     bfm_stream_t stream) {
    if (!g || !arg || !dst || C <= 0 || D < 4 || H < 4 || W < 4) return BFM_E_ARG;
    const int Pd = D / 4, Ph = H / 4, Pw = W / 4;
    if (accumulate) {
        const int64_t n = (int64_t)Pd * Ph * Pw * C;
        hipLaunchKernelGGL(maxpool4_bwd_scatter_kernel, dim3(nblk(n)), dim3(NT), 0, bfm_s(stream), g, arg, C, H, W, Ph, Pw,
                           dst, n);
    } else {
        const int64_t n = (int64_t)D * H * W * C;
        hipLaunchKernelGGL(maxpool4_bwd_gather_kernel, dim3(nblk(n)), dim3(NT), 0, bfm_s(stream), g, arg, C, H, W, Pd, Ph,
                           Pw, dst, n);
    }
    return bfm_launch_status();
}

int bfm_age_conv_fwd(const float* x, int Cin, int D, int H, int W, const float* w, const float* b, int Cout, float* y,
                     bfm_stream_t stream) {
    if (!x || !w || !b || !y || Cin <= 0 || D <= 0 || H <= 0 || W <= 0) return BFM_E_ARG;
    if (Cout <= 0 || Cout % CPT) return BFM_E_SHAPE;
    const int64_t n = (int64_t)D * H * W * (Cout / CPT);
    hipLaunchKernelGGL(conv_fwd_kernel, dim3(nblk(n)), dim3(NT), 0, bfm_s(stream), x, Cin, D, H, W, w, b, Cout, y, n);
    return bfm_launch_status();
}

size_t bfm_age_conv_bwd_workspace(int Cin, int D, int H, int W, int Cout) {
    if (Cin <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)conv_bwd_chunks(D, H, W) * Cout * (Cin + 1) * 27 * sizeof(float);
}

int bfm_age_conv_bwd(const float* x, int Cin, int D, int H, int W, const float* w, int Cout, const float* y, const float* dy,
                     float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (!x || !w || !dy || !dw || !db || Cin <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return BFM_E_ARG;
    if (!workspace || workspace_bytes < bfm_age_conv_bwd_workspace(Cin, D, H, W, Cout)) return BFM_E_WORKSPACE;
    const int64_t nvox = (int64_t)D * H * W;
    const int nb_dgrad = dx ? (int)nblk(nvox * Cin) : 0;
    const int tiles = bfm_cdiv(Cout * (Cin + 1), NT);
    const int nchunks = (int)conv_bwd_chunks(D, H, W);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(conv_bwd_kernel, dim3(nb_dgrad + nchunks * tiles), dim3(NT), 0, bfm_s(stream), x, Cin, D, H, W, w,
                       Cout, y, dy, dx, nb_dgrad, tiles, part);
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(nblk(Cout * Cin * 27 + Cout)), dim3(NT), 0, bfm_s(stream), part,
                       nchunks, Cin, Cout, dw, db);
    return bfm_launch_status();
}

int bfm_age_mlp_fwd(const float* y2, int nv, const bfm_age_params_t* prm, int n_flat, float* h1, float* h2, float* out,
                    bfm_stream_t stream) {
    if (!y2 || !prm || !h1 || !h2 || !out || nv <= 0) return BFM_E_ARG;
    if (!prm->l1w || !prm->l1b || !prm->l2w || !prm->l2b || !prm->l3w || !prm->l3b) return BFM_E_ARG;
    if (n_flat != 4 * nv) return BFM_E_SHAPE;
    hipLaunchKernelGGL(mlp1_kernel, dim3(H1), dim3(NT), 0, bfm_s(stream), y2, nv, prm->l1w, prm->l1b, n_flat, h1);
    hipLaunchKernelGGL(mlp23_kernel, dim3(1), dim3(64), 0, bfm_s(stream), h1, prm->l2w, prm->l2b, prm->l3w, prm->l3b, h2, out);
    return bfm_launch_status();
}

size_t bfm_age_mlp_bwd_workspace(void) { return H1 * sizeof(float); }

int bfm_age_mlp_bwd(const float* y2, int nv, const bfm_age_params_t* prm, int n_flat, const float* h1, const float* h2,
                    const float* p, const float* dp_in, double age, float coef, double* loss, const bfm_age_grads_t* grd,
                    float* dy2, void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (!y2 || !prm || !h1 || !h2 || !p || !grd || !dy2 || nv <= 0) return BFM_E_ARG;
    if (!prm->l1w || !prm->l2w || !prm->l3w) return BFM_E_ARG;
    if (!grd->l1w || !grd->l1b || !grd->l2w || !grd->l2b || !grd->l3w || !grd->l3b) return BFM_E_ARG;
    if (n_flat != 4 * nv) return BFM_E_SHAPE;
    if (!workspace || workspace_bytes < bfm_age_mlp_bwd_workspace()) return BFM_E_WORKSPACE;
    float* dpre1 = static_cast<float*>(workspace);
    hipLaunchKernelGGL(mlp_bwd_small_kernel, dim3(1), dim3(NT), 0, bfm_s(stream), h1, h2, p, dp_in, age, coef, loss, prm->l2w,
                       prm->l3w, grd->l1b, grd->l2w, grd->l2b, grd->l3w, grd->l3b, dpre1);
    hipLaunchKernelGGL(mlp_bwd_l1_kernel, dim3(nblk(n_flat)), dim3(NT), 0, bfm_s(stream), y2, nv, prm->l1w, n_flat, dpre1,
                       grd->l1w, dy2);
    return bfm_launch_status();
}

}  // extern "C"
