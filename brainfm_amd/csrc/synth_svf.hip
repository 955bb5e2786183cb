// The generator's surface task (Generator/datasets.py:202-226, Generator/utils.py:479-531):
//
//   svf_integrate   : scaling and squaring of the nonlinear field in both directions, n steps of
//                     Fsvf += fast_3D_interp_torch(Fsvf, xx + Fsvf[...,0], yy + Fsvf[...,1], zz + Fsvf[...,2], 'linear')
//                     from Fsvf = F * s and from Fsvf_neg = -F * s, s = 1 / 2**n
//   deform_vertices : read_and_deform_surface's per-vertex arithmetic for up to four vertex sets:
//                     V -= c2; V = V @ inv(A).T; V += fast_3D_interp_torch(Fneg, V + c2); V += c2; optional x-flip
//
// One thread per voxel / vertex.  The gathers are gather3d.h's (the texel policy, validity test, corners and lerp chain of
// bfm_interp3d_linear), so each voxel's arithmetic is fast_3D_interp_torch's, in its order; with -ffp-contract=off the fp32
// results are the reference's bits.  The interpolation of a step is complete before its add in the reference, so a step
// reads one buffer and writes another (ping-pong); nothing is updated in place.  No atomics, no packed FP32.
#include "bfm_common.h"
#include "gather3d.h"

namespace {

struct SvfDir {
    const float* src;   // [nx][ny][nz][3]: the field of the previous step (F itself on the first step)
    float* dst;
    float m;            // FIRST: the field is m * src (m = +-s); the texels are scaled before the lerp
};
struct SvfDirs { SvfDir d[2]; };

// blockIdx.y = direction
template <bool FIRST>
__global__ void __launch_bounds__(256) svf_step(SvfDirs P, int nx, int ny, int nz, uint32_t vbytes) {
    const SvfDir D = P.d[blockIdx.y];
    const __amdgpu_buffer_rsrc_t R = tex_rsrc(D.src, vbytes);
    const int64_t n = (int64_t)nx * ny * nz;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % nz);
        const int y = (int)((i / nz) % ny);
        const int x = (int)(i / ((int64_t)ny * nz));
        float v0 = D.src[i * 3 + 0], v1 = D.src[i * 3 + 1], v2 = D.src[i * 3 + 2];
        if constexpr (FIRST) { v0 = v0 * D.m; v1 = v1 * D.m; v2 = v2 * D.m; }
        float r[3];
        interp3_c3<FIRST>(R, nx, ny, nz, (float)x + v0, (float)y + v1, (float)z + v2, D.m, r);
        // Fsvf += Y with Y = 0 where not ok: the add is made there too (-0 + 0 = +0)
        D.dst[i * 3 + 0] = v0 + r[0];
        D.dst[i * 3 + 1] = v1 + r[1];
        D.dst[i * 3 + 2] = v2 + r[2];
    }
}

// n = 0: F * 1 and -F * 1
__global__ void __launch_bounds__(256) svf_scale(SvfDirs P, int64_t n3) {
    const SvfDir D = P.d[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x)
        D.dst[i] = D.src[i] * D.m;
}

struct VertParams {
    float* V[BFM_VERTEX_SETS_MAX];
    int64_t n[BFM_VERTEX_SETS_MAX];
    float ainv[9], c2[3];
    float flip_hi;      // size[0] - 1
    int flip;
};

// blockIdx.y = vertex set
__global__ void __launch_bounds__(256) deform_vertices_k(const float* __restrict__ Fneg, int nx, int ny, int nz,
                                                        uint32_t vbytes, VertParams P) {
    float* V = P.V[blockIdx.y];
    const int64_t n = P.n[blockIdx.y];
    const __amdgpu_buffer_rsrc_t R = tex_rsrc(Fneg, vbytes);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float u0 = V[i * 3 + 0] - P.c2[0], u1 = V[i * 3 + 1] - P.c2[1], u2 = V[i * 3 + 2] - P.c2[2];
        float w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = (P.ainv[k * 3 + 0] * u0 + P.ainv[k * 3 + 1] * u1) + P.ainv[k * 3 + 2] * u2;
        float g[3];
        interp3_c3<false>(R, nx, ny, nz, w[0] + P.c2[0], w[1] + P.c2[1], w[2] + P.c2[2], 1.f, g);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = (w[k] + g[k]) + P.c2[k];
        if (P.flip) w[0] = P.flip_hi - w[0];
        V[i * 3 + 0] = w[0]; V[i * 3 + 1] = w[1]; V[i * 3 + 2] = w[2];
    }
}

inline int blocks_for(int64_t n) {
    const int64_t b = bfm_cdiv64(n, 256);
    return (int)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

}  // namespace

extern "C" size_t bfm_svf_integrate_workspace(int sx, int sy, int sz) {
    if (sx <= 0 || sy <= 0 || sz <= 0) return 0;
    return (size_t)2 * sx * sy * sz * 3 * sizeof(float);
}

extern "C" int bfm_svf_integrate(const float* F, int sx, int sy, int sz, int n_steps, float* F_out, float* Fneg_out,
                                 void* workspace, size_t workspace_bytes, bfm_stream_t stream) {
    if (!F || !F_out || !Fneg_out || sx <= 0 || sy <= 0 || sz <= 0 || n_steps < 0 || n_steps > 62) return BFM_E_ARG;
    const int64_t n = (int64_t)sx * sy * sz;
    if (n * 12 >= ((int64_t)1 << 32)) return BFM_E_SHAPE;            // 32-bit byte offsets of the texel loads
    const float s = (float)(1.0 / (double)((uint64_t)1 << n_steps));
    hipStream_t st = bfm_s(stream);
    if (n_steps == 0) {
        SvfDirs P{{{F, F_out, 1.f}, {F, Fneg_out, -1.f}}};
        hipLaunchKernelGGL(svf_scale, dim3(blocks_for(n * 3), 2), dim3(256), 0, st, P, n * 3);
        return bfm_launch_status();
    }
    if (n_steps > 1 && (!workspace || workspace_bytes < bfm_svf_integrate_workspace(sx, sy, sz))) return BFM_E_WORKSPACE;
    float* scratch[2] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + n * 3};
    float* out[2] = {F_out, Fneg_out};
    const uint32_t vbytes = (uint32_t)(n * 12);
    const float* src[2] = {F, F};
    // step k (1..n) writes the output when n - k is even, the scratch buffer otherwise: the last step lands in the output
    for (int k = 1; k <= n_steps; ++k) {
        const bool to_out = ((n_steps - k) & 1) == 0;
        SvfDirs P{{{src[0], to_out ? out[0] : scratch[0], s}, {src[1], to_out ? out[1] : scratch[1], -s}}};
        if (k == 1)
            hipLaunchKernelGGL(svf_step<true>, dim3(blocks_for(n), 2), dim3(256), 0, st, P, sx, sy, sz, vbytes);
        else
            hipLaunchKernelGGL(svf_step<false>, dim3(blocks_for(n), 2), dim3(256), 0, st, P, sx, sy, sz, vbytes);
        src[0] = P.d[0].dst; src[1] = P.d[1].dst;
    }
    return bfm_launch_status();
}

extern "C" int bfm_deform_vertices(const float* Fneg, int sx, int sy, int sz, const bfm_vertex_set_t* sets, int n_sets,
                                   const float* Ainv_host, const float* c2_host, int flip, int size0, bfm_stream_t stream) {
    if (!Fneg || !sets || !Ainv_host || !c2_host || sx <= 0 || sy <= 0 || sz <= 0 || n_sets < 1 ||
        n_sets > BFM_VERTEX_SETS_MAX)
        return BFM_E_ARG;
    const int64_t nv = (int64_t)sx * sy * sz;
    if (nv * 12 >= ((int64_t)1 << 32)) return BFM_E_SHAPE;
    VertParams P{};
    int64_t nmax = 0;
    for (int j = 0; j < n_sets; ++j) {
        if (sets[j].n < 0 || (sets[j].n > 0 && !sets[j].V)) return BFM_E_ARG;
        P.V[j] = sets[j].V;
        P.n[j] = sets[j].n;
        nmax = std::max(nmax, sets[j].n);
    }
    for (int i = 0; i < 9; ++i) P.ainv[i] = Ainv_host[i];
    for (int i = 0; i < 3; ++i) P.c2[i] = c2_host[i];
    P.flip = flip ? 1 : 0;
    P.flip_hi = (float)(size0 - 1);
    if (nmax == 0) return BFM_OK;
    hipLaunchKernelGGL(deform_vertices_k, dim3(blocks_for(nmax), n_sets), dim3(256), 0, bfm_s(stream), Fneg, sx, sy, sz,
                       (uint32_t)(nv * 12), P);
    return bfm_launch_status();
}
