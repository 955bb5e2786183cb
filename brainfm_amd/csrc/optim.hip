// The optimisers Trainer/models/__init__.py:362-372 (build_optimizer) offers: torch.optim.AdamW, torch.optim.Adam,
// torch.optim.SGD (momentum 0.9) and the Barlow-Twins LARS of utils/misc.py:1279-1317, each over ALL parameters of the step in
// one launch, the clip norms that precede them (bfm_grad_sumsq_multi; for LARS bfm_lars_sums_multi), and the single-tensor
// bfm_adamw_step of the C ABI.
//
// The multi-tensor form: one workgroup of 256 threads owns one chunk (chunk_elems elements, a multiple of 4) of one tensor;
// descriptors (bfm_optim_tensor_t) and the chunk map live in device memory.  A chunk runs on 16-byte accesses where every
// pointer of its tensor is 16-byte aligned and the chunk's length is a multiple of 4, and element by element otherwise
// (head weights and biases are views into head_w / head_b at arbitrary float offsets).  Sums are fp64 per lane, then a fixed
// tree per block, then the block partials of a tensor folded in a fixed order by one wave: no float atomics, the same bits on
// every run.  The two measuring kernels keep a block tree each (the LDS halving of block_sum for the sum of squares, the wave
// butterfly for LARS' three sums): the trees round differently in the last bit, the norms feed the update, and
// tests/test_gpu_optim_bits.py holds both to their stored bits.  The kernels stream: 5 (SGD, LARS) or 7 (Adam, AdamW) floats
// move per parameter and nothing is reused.
#include "bfm_common.h"

namespace {

enum { OPT_ADAM = 0, OPT_SGD = 1, OPT_LARS = 2, OPT_ADAMW = 3 };

struct OptimArgs {
    float lr, b1, b2, omb1, omb2, eps, wd, mom;   // omb = 1 - beta of Adam, rounded once from the double (bfm_adam_step_multi)
};

// One element.  s0 = exp_avg | momentum_buffer | mu, s1 = exp_avg_sq (Adam and AdamW).
template <int KIND>
__device__ __forceinline__ void optim_one(float& p, float g, float& s0, float& s1, const bfm_optim_tensor_t& d,
                                          const OptimArgs& a) {
    if (KIND == OPT_ADAMW) {
        // adamw_kernel's expressions in its order (every checkpoint written so far holds their bits): 1 - beta is formed in
        // float, and 1.f - 0.999f is 1.3e-5 below 1e-3, so exp_avg_sq is low by that share
        g = g * d.grad_scale;
        p = p * (1.f - a.lr * a.wd);
        s0 = a.b1 * s0 + (1.f - a.b1) * g;
        s1 = a.b2 * s1 + (1.f - a.b2) * g * g;
        const float denom = sqrtf(s1) / d.bias2_sqrt + a.eps;
        p = p - (a.lr / d.bias1) * (s0 / denom);
    } else if (KIND == OPT_ADAM) {
        // torch.optim.Adam (amsgrad off, maximize off): the decay joins the gradient; then AdamW's expressions, but for
        // 1 - beta, which comes rounded once from the double as torch hands it over
        g = d.grad_scale * g + a.wd * p;
        s0 = a.b1 * s0 + a.omb1 * g;
        s1 = a.b2 * s1 + a.omb2 * g * g;
        const float denom = sqrtf(s1) / d.bias2_sqrt + a.eps;
        p = p - (a.lr / d.bias1) * (s0 / denom);
    } else if (KIND == OPT_SGD) {
        // torch.optim.SGD(momentum, dampening 0, nesterov off); a zero buffer gives torch's first step (buf = g)
        g = d.grad_scale * g + a.wd * p;
        s0 = a.mom * s0 + g;
        p = p - a.lr * s0;
    } else {
        // utils/misc.py:1296-1317.  d.wd and d.q are the tensor's own: 0 and 1 for a parameter the reference sees as 1-D
        float dp = d.grad_scale * g;
        if (d.wd != 0.f) dp = dp + d.wd * p;
        dp = dp * d.q;
        s0 = a.mom * s0 + dp;
        p = p - a.lr * s0;
    }
}

// U: how many 16-byte rows of every stream a thread requests before it uses the first.  AdamW runs at 1, the depth its kernel
// always had: at 4 it measured 1.2 % slower (profiles/optim_unify.txt).
template <int KIND, int U = 4>
__global__ void __launch_bounds__(256) optim_multi_kernel(const bfm_optim_tensor_t* __restrict__ T,
                                                          const int32_t* __restrict__ chunk_tensor, int64_t chunk_elems,
                                                          OptimArgs a) {
    constexpr bool TWO = KIND == OPT_ADAM || KIND == OPT_ADAMW;
    const int t = chunk_tensor[blockIdx.x];
    const bfm_optim_tensor_t d = T[t];
    const int64_t i0 = (int64_t)(blockIdx.x - d.first_chunk) * chunk_elems, i1 = min(d.n, i0 + chunk_elems);
    if (i0 >= i1) return;
    uintptr_t al = reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.s0);
    if (TWO) al |= reinterpret_cast<uintptr_t>(d.s1);
    if ((al & 15) == 0 && ((i1 - i0) & 3) == 0) {
        float4* p4 = reinterpret_cast<float4*>(d.p + i0);
        const float4* g4 = reinterpret_cast<const float4*>(d.g + i0);
        float4* a4 = reinterpret_cast<float4*>(d.s0 + i0);
        float4* b4 = TWO ? reinterpret_cast<float4*>(d.s1 + i0) : nullptr;
        const int64_t n4 = (i1 - i0) >> 2;
        for (int64_t base = threadIdx.x; base < n4; base += 256 * U) {
            float4 pp[U], gg[U], aa[U], bb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + 256 * u;
                if (i < n4) {
                    pp[u] = p4[i];
                    gg[u] = g4[i];
                    aa[u] = a4[i];
                    if (TWO) bb[u] = b4[i];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + 256 * u;
                if (i < n4) {
                    if (!TWO) bb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    optim_one<KIND>(pp[u].x, gg[u].x, aa[u].x, bb[u].x, d, a);
                    optim_one<KIND>(pp[u].y, gg[u].y, aa[u].y, bb[u].y, d, a);
                    optim_one<KIND>(pp[u].z, gg[u].z, aa[u].z, bb[u].z, d, a);
                    optim_one<KIND>(pp[u].w, gg[u].w, aa[u].w, bb[u].w, d, a);
                    p4[i] = pp[u];
                    a4[i] = aa[u];
                    if (TWO) b4[i] = bb[u];
                }
            }
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
            float pi = d.p[i], ai = d.s0[i], bi = TWO ? d.s1[i] : 0.f;
            optim_one<KIND>(pi, d.g[i], ai, bi, d, a);
            d.p[i] = pi;
            d.s0[i] = ai;
            if (TWO) d.s1[i] = bi;
        }
    }
}

// torch.optim.AdamW on one tensor (bfm_adamw_step): p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
// p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
__global__ void adamw_kernel(bfm_optim_tensor_t d, OptimArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = d.p[i], mi = d.s0[i], vi = d.s1[i];
        optim_one<OPT_ADAMW>(pi, d.g[i], mi, vi, d, a);
        d.p[i] = pi;
        d.s0[i] = mi;
        d.s1[i] = vi;
    }
}

__device__ __forceinline__ double block_sum(double v, double* red) {        // 256 threads, fixed tree
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// The clip norms' measuring pass (clip_gradients / GradScaler.unscale_): per chunk the sum of g^2 in fp64 and the non-finite
// flag of g.  part: [nchunks].
__global__ void __launch_bounds__(256) sumsq_multi_kernel(const bfm_optim_tensor_t* __restrict__ T,
                                                          const int32_t* __restrict__ chunk_tensor, int64_t chunk_elems,
                                                          double* __restrict__ part, int* __restrict__ nonfinite) {
    __shared__ double red[256];
    const int t = chunk_tensor[blockIdx.x];
    const bfm_optim_tensor_t d = T[t];
    const int64_t i0 = (int64_t)(blockIdx.x - d.first_chunk) * chunk_elems, i1 = min(d.n, i0 + chunk_elems);
    const float* g = d.g;
    double acc = 0.0;
    bool bad = false;
    if (((reinterpret_cast<uintptr_t>(g) & 15) == 0) && ((i1 - i0) & 3) == 0) {
        const float4* g4 = reinterpret_cast<const float4*>(g + i0);
        for (int64_t i = threadIdx.x; i < (i1 - i0) >> 2; i += 256) {
            const float4 x = g4[i];
            if (!(fabsf(x.x) <= 3.402823466e+38f) || !(fabsf(x.y) <= 3.402823466e+38f) || !(fabsf(x.z) <= 3.402823466e+38f) ||
                !(fabsf(x.w) <= 3.402823466e+38f))
                bad = true;
            acc += (double)x.x * (double)x.x + (double)x.y * (double)x.y + (double)x.z * (double)x.z + (double)x.w * (double)x.w;
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
            const float x = g[i];
            if (!(fabsf(x) <= 3.402823466e+38f)) bad = true;
            acc += (double)x * (double)x;
        }
    }
    if (bad) atomicOr(nonfinite, 1);
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// one wave per tensor: lane l adds the partials of chunks l, l + 64, ... in ascending order, then the butterfly
__global__ void __launch_bounds__(64) sumsq_multi_fold_kernel(const bfm_optim_tensor_t* __restrict__ T, int ntensors,
                                                              int64_t chunk_elems, const double* __restrict__ part,
                                                              double* __restrict__ out) {
    const int t = blockIdx.x, l = threadIdx.x;
    if (t >= ntensors) return;
    const int c0 = T[t].first_chunk, nc = (int)((T[t].n + chunk_elems - 1) / chunk_elems);
    double s_ = 0.0;
    for (int c = l; c < nc; c += 64) s_ += part[c0 + c];
    s_ = wave_reduce_sum(s_);
    if (l == 0) out[t] = s_;
}

// LARS' measuring pass: per chunk { sum g^2, sum p^2, sum p g } in fp64 and the non-finite flag of g.  part: [nchunks][3].
__global__ void __launch_bounds__(256) lars_sums_multi_kernel(const bfm_optim_tensor_t* __restrict__ T,
                                                              const int32_t* __restrict__ chunk_tensor, int64_t chunk_elems,
                                                              double* __restrict__ part, int* __restrict__ nonfinite) {
    __shared__ double red[3][4];
    const int t = chunk_tensor[blockIdx.x];
    const bfm_optim_tensor_t d = T[t];
    const int64_t i0 = (int64_t)(blockIdx.x - d.first_chunk) * chunk_elems, i1 = min(d.n, i0 + chunk_elems);
    double sgg = 0.0, spp = 0.0, spg = 0.0;
    bool bad = false;
    auto one = [&](float pf, float gf) __attribute__((always_inline)) {
        if (!(fabsf(gf) <= 3.402823466e+38f)) bad = true;
        const double p = (double)pf, g = (double)gf;
        sgg += g * g;
        spp += p * p;
        spg += p * g;
    };
    const uintptr_t al = reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g);
    if (i0 < i1 && (al & 15) == 0 && ((i1 - i0) & 3) == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(d.p + i0);
        const float4* g4 = reinterpret_cast<const float4*>(d.g + i0);
        const int64_t n4 = (i1 - i0) >> 2;
        constexpr int U = 4;
        for (int64_t base = threadIdx.x; base < n4; base += 256 * U) {
            float4 pp[U], gg[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + 256 * u;
                if (i < n4) {
                    pp[u] = p4[i];
                    gg[u] = g4[i];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (base + 256 * u < n4) {
                    one(pp[u].x, gg[u].x);
                    one(pp[u].y, gg[u].y);
                    one(pp[u].z, gg[u].z);
                    one(pp[u].w, gg[u].w);
                }
            }
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) one(d.p[i], d.g[i]);
    }
    if (bad) atomicOr(nonfinite, 1);
    // a fixed tree: the wave's butterfly, then the four waves in order
    sgg = wave_reduce_sum(sgg);
    spp = wave_reduce_sum(spp);
    spg = wave_reduce_sum(spg);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = sgg;
        red[1][w] = spp;
        red[2][w] = spg;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double* r = red[threadIdx.x];
        part[(int64_t)blockIdx.x * 3 + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// one wave per tensor: lane l adds the partials of chunks l, l + 64, ... in ascending order, then the butterfly
__global__ void __launch_bounds__(64) lars_sums_fold_kernel(const bfm_optim_tensor_t* __restrict__ T, int ntensors,
                                                            int64_t chunk_elems, const double* __restrict__ part,
                                                            double* __restrict__ out) {
    const int t = blockIdx.x, l = threadIdx.x;
    if (t >= ntensors) return;
    const int c0 = T[t].first_chunk, nc = (int)((T[t].n + chunk_elems - 1) / chunk_elems);
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = l; c < nc; c += 64)
        for (int j = 0; j < 3; ++j) s[j] += part[(int64_t)(c0 + c) * 3 + j];
    for (int j = 0; j < 3; ++j) s[j] = wave_reduce_sum(s[j]);
    if (l == 0)
        for (int j = 0; j < 3; ++j) out[(int64_t)t * 3 + j] = s[j];
}

bool bad_multi_args(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                    int64_t chunk_elems) {
    return !tensors || !chunk_tensor || ntensors <= 0 || nchunks <= 0 || chunk_elems <= 0 || (chunk_elems & 3);
}

}  // namespace

extern "C" int bfm_grad_sumsq_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                                    int64_t chunk_elems, double* sums_out, int32_t* nonfinite, void* workspace,
                                    size_t workspace_bytes, bfm_stream_t stream) {
    if (bad_multi_args(tensors, ntensors, chunk_tensor, nchunks, chunk_elems) || !sums_out || !nonfinite || !workspace)
        return BFM_E_ARG;
    if (workspace_bytes < (size_t)nchunks * sizeof(double)) return BFM_E_WORKSPACE;
    hipStream_t st = bfm_s(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(sumsq_multi_kernel, dim3(nchunks), dim3(256), 0, st, tensors, chunk_tensor, chunk_elems, part, nonfinite);
    hipLaunchKernelGGL(sumsq_multi_fold_kernel, dim3(ntensors), dim3(64), 0, st, tensors, ntensors, chunk_elems, part, sums_out);
    return bfm_launch_status();
}

extern "C" int bfm_adamw_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                                    int64_t chunk_elems, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    bfm_stream_t stream) {
    if (bad_multi_args(tensors, ntensors, chunk_tensor, nchunks, chunk_elems)) return BFM_E_ARG;
    const OptimArgs a{lr, beta1, beta2, 0.f, 0.f, eps, weight_decay, 0.f};
    hipLaunchKernelGGL((optim_multi_kernel<OPT_ADAMW, 1>), dim3(nchunks), dim3(256), 0, bfm_s(stream), tensors, chunk_tensor,
                       chunk_elems, a);
    return bfm_launch_status();
}

extern "C" int bfm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, int step, float grad_scale, bfm_stream_t stream) {
    if (!p || !g || !m || !v || n <= 0 || step < 1) return BFM_E_ARG;
    const bfm_optim_tensor_t d{p, g, m, v, n, grad_scale, 1.f - powf(beta1, (float)step), sqrtf(1.f - powf(beta2, (float)step)),
                               0, 1.f, 0.f};
    const OptimArgs a{lr, beta1, beta2, 0.f, 0.f, eps, weight_decay, 0.f};
    const int nb = (int)std::min<int64_t>(4096, bfm_cdiv64(n, 256));
    hipLaunchKernelGGL(adamw_kernel, dim3(nb), dim3(256), 0, bfm_s(stream), d, a);
    return bfm_launch_status();
}

extern "C" int bfm_adam_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                                   int64_t chunk_elems, float lr, double beta1, double beta2, float eps, float weight_decay,
                                   bfm_stream_t stream) {
    if (bad_multi_args(tensors, ntensors, chunk_tensor, nchunks, chunk_elems)) return BFM_E_ARG;
    // torch hands its kernels 1 - beta formed in double; 1.f - (float)0.999 would be 1.3e-5 off
    const OptimArgs a{lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, 0.f};
    hipLaunchKernelGGL(optim_multi_kernel<OPT_ADAM>, dim3(nchunks), dim3(256), 0, bfm_s(stream), tensors, chunk_tensor,
                       chunk_elems, a);
    return bfm_launch_status();
}

extern "C" int bfm_sgd_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                                  int64_t chunk_elems, float lr, float momentum, float weight_decay, bfm_stream_t stream) {
    if (bad_multi_args(tensors, ntensors, chunk_tensor, nchunks, chunk_elems)) return BFM_E_ARG;
    const OptimArgs a{lr, 0.f, 0.f, 0.f, 0.f, 0.f, weight_decay, momentum};
    hipLaunchKernelGGL(optim_multi_kernel<OPT_SGD>, dim3(nchunks), dim3(256), 0, bfm_s(stream), tensors, chunk_tensor,
                       chunk_elems, a);
    return bfm_launch_status();
}

extern "C" int bfm_lars_sums_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                                   int64_t chunk_elems, double* sums_out, int32_t* nonfinite, void* workspace,
                                   size_t workspace_bytes, bfm_stream_t stream) {
    if (bad_multi_args(tensors, ntensors, chunk_tensor, nchunks, chunk_elems) || !sums_out || !nonfinite || !workspace)
        return BFM_E_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return BFM_E_ARG;
    if (workspace_bytes < (size_t)nchunks * 3 * sizeof(double)) return BFM_E_WORKSPACE;
    hipStream_t st = bfm_s(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(lars_sums_multi_kernel, dim3(nchunks), dim3(256), 0, st, tensors, chunk_tensor, chunk_elems, part,
                       nonfinite);
    hipLaunchKernelGGL(lars_sums_fold_kernel, dim3(ntensors), dim3(64), 0, st, tensors, ntensors, chunk_elems, part, sums_out);
    return bfm_launch_status();
}

extern "C" int bfm_lars_step_multi(const bfm_optim_tensor_t* tensors, int ntensors, const int32_t* chunk_tensor, int nchunks,
                                   int64_t chunk_elems, float lr, float momentum, bfm_stream_t stream) {
    if (bad_multi_args(tensors, ntensors, chunk_tensor, nchunks, chunk_elems)) return BFM_E_ARG;
    const OptimArgs a{lr, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, momentum};
    hipLaunchKernelGGL(optim_multi_kernel<OPT_LARS>, dim3(nchunks), dim3(256), 0, bfm_s(stream), tensors, chunk_tensor,
                       chunk_elems, a);
    return bfm_launch_status();
}
