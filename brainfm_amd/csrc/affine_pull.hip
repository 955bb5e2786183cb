// Resampling through a 3 x 4 voxel-to-voxel matrix (brainfm_amd/native.py): the maps an inference flow leaves on the
// processed grid are pulled onto the voxel grid of the scan the user handed in.  resize -> align -> crop is affine in
// voxel coordinates, so the source coordinate of a destination voxel comes from twelve doubles in the kernel arguments
// and no grid tensor exists (affine_grid + grid_pull would write and re-read 12 bytes per voxel and map).
//
// Coordinates are fp64 on the device, x_r = ((M[r][0] * i + M[r][1] * j) + M[r][2] * k) + M[r][3], every product and sum
// rounded on its own (the library is built with -ffp-contract=off), so NumPy float64 reproduces them bit for bit; an fp32
// coordinate is off by up to 3e-5 voxels at these extents, enough to move a nearest-neighbour label.
//
// Linear: f = floor(x), wc = (float)(x - f), wf = 1.f - wc per axis, the eight corners f, f + 1, a corner outside the
// source is a texel of 0 (grid_sample's padding_mode='zeros', align_corners=True), combined by gather3d.h's trilin_lerp
// chain, so NumPy float32 reproduces the value bit for bit.  Nearest: floor(x + 0.5) per axis, the 4-byte pattern copied,
// 0 outside.
//
// Load policy: ordinary loads, not gather3d.h's ld_tex.  The addresses are not data dependent -- a lane's neighbours read
// the neighbouring texels of an affine image of the destination row -- so the lines a wave touches are the ones its
// neighbours need next, and the L1 that ld_tex's sc1 loads go past is what serves them.
#include "gather3d.h"

namespace {

struct AffM { double m[12]; };

// floor(x) and the weights of one axis.  x is known to lie in (-1, n), so the conversion to int is exact.
__device__ __forceinline__ void axis_setup(double x, int& f, float& wc, float& wf) {
    const double fl = floor(x);
    f = (int)fl;
    wc = (float)(x - fl);
    wf = 1.f - wc;
}

__device__ __forceinline__ double affine_row(const AffM& A, int r, double i, double j, double k) {
    return ((A.m[4 * r] * i + A.m[4 * r + 1] * j) + A.m[4 * r + 2] * k) + A.m[4 * r + 3];
}

// The footprint of one destination voxel in a (D,H,W) source whose last axis has element stride `sw`: element offsets
// of the eight corners (tXYZ order of trilin_lerp: 000 100 010 110 001 101 011 111, X the FIRST source axis), which of
// them lie inside, and the weights.  any == false: the whole footprint is outside (or a coordinate is NaN).
struct Foot {
    Trilin t;
    int64_t off[8];
    bool in[8];
    bool any;
};
__device__ __forceinline__ Foot foot_setup(double x, double y, double z, int D, int H, int W, int64_t sw) {
    Foot F;
    F.any = (x > -1.0) && (x < (double)D) && (y > -1.0) && (y < (double)H) && (z > -1.0) && (z < (double)W);
    if (!F.any) return F;
    axis_setup(x, F.t.fx, F.t.wcx, F.t.wfx);
    axis_setup(y, F.t.fy, F.t.wcy, F.t.wfy);
    axis_setup(z, F.t.fz, F.t.wcz, F.t.wfz);
    F.t.cx = F.t.fx + 1; F.t.cy = F.t.fy + 1; F.t.cz = F.t.fz + 1;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ix = (c & 1) ? F.t.cx : F.t.fx, iy = (c & 2) ? F.t.cy : F.t.fy, iz = (c & 4) ? F.t.cz : F.t.fz;
        F.in[c] = ix >= 0 && ix < D && iy >= 0 && iy < H && iz >= 0 && iz < W;
        F.off[c] = (((int64_t)ix * H + iy) * W + iz) * sw;
    }
    return F;
}
__device__ __forceinline__ float foot_lerp(const Foot& F, const float* __restrict__ s) {
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = F.in[c] ? s[F.off[c]] : 0.f;
    return trilin_lerp(F.t, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
}

// out [K][X][Y][Z] <- src [K] maps of (D,H,W), map k at src + k * map_stride.  One thread per destination voxel, lanes
// along z; the K maps share the thread's indices and weights.  nearest_mask bit k: map k is pulled by nearest neighbour.
__global__ void __launch_bounds__(256) affine_pull_multi(const float* __restrict__ src, int64_t map_stride, int K, int D,
                                                         int H, int W, AffM A, uint64_t nearest_mask, int X, int Y, int Z,
                                                         float* __restrict__ out) {
    const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (k >= Z || j >= Y) return;
    const int64_t nvox = (int64_t)X * Y * Z;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1;
    for (int i = blockIdx.z; i < X; i += gridDim.z) {
        const double x = affine_row(A, 0, i, j, k), y = affine_row(A, 1, i, j, k), z = affine_row(A, 2, i, j, k);
        const int64_t o = ((int64_t)i * Y + j) * Z + k;
        Foot F{};
        if (nearest_mask != all) F = foot_setup(x, y, z, D, H, W, 1);
        int64_t noff = -1;
        if (nearest_mask) {
            const double rx = floor(x + 0.5), ry = floor(y + 0.5), rz = floor(z + 0.5);
            if (rx >= 0.0 && rx < (double)D && ry >= 0.0 && ry < (double)H && rz >= 0.0 && rz < (double)W)
                noff = ((int64_t)rx * H + (int64_t)ry) * W + (int64_t)rz;
        }
        for (int m = 0; m < K; ++m) {
            const float* s = src + (int64_t)m * map_stride;
            if ((nearest_mask >> m) & 1) {
                const uint32_t bits = noff >= 0 ? reinterpret_cast<const uint32_t*>(s)[noff] : 0u;
                reinterpret_cast<uint32_t*>(out)[(int64_t)m * nvox + o] = bits;
            } else {
                out[(int64_t)m * nvox + o] = F.any ? foot_lerp(F, s) : 0.f;
            }
        }
    }
}

// label [X][Y][Z] <- lut[first strict maximum over c of the interpolated posterior c], post (D,H,W,C) channels-last.
// G lanes (a power of two, 1..64) share a destination voxel and take channels lane, lane + G, ...: each corner is then
// one contiguous read of the voxel's C-vector, and the winner comes from a G-wide butterfly on (value, channel).  A block
// covers max(64, 256 / G) voxels of one z row; its four waves step through them 256 / G at a time.  G = 1 is one thread
// per voxel looping over the channels: coalesced stores, but every load instruction touches 64 C-vectors.
// Every lane forms the coordinates, offsets and weights of its voxel, so a wide G repeats that work in more lanes per
// voxel while a narrow one spreads a load over more C-vectors.  Measured at 256^3 -> 320 x 320 x 256, cold
// (scripts/bench_native.py, profiles/native.txt), G = 1 / 4 / 8 / 16 / 32 / 64: C = 56 123 / 13.8 / 7.1 / 6.4 / 10.4 / 19.1 ms,
// C = 18 8.8 / 2.0 / 2.8 / 5.2 / 9.4 / 18.9 ms.  Both optima are the narrowest width at which a lane takes at most five
// channels, and nothing wider than 16 won anywhere: that is bfm_affine_pull_route.  C <= 5 (one thread per voxel, whose
// neighbours' C-vectors are contiguous) has not been timed.
// The winner is the first channel whose value is > 0 and > every earlier one: ties go to the lower channel, a NaN loses
// every comparison and so never wins, and a voxel with no positive value (outside the field of view included) gets 0.
__global__ void __launch_bounds__(256) affine_pull_argmax(const float* __restrict__ post, int C, int D, int H, int W,
                                                          const int32_t* __restrict__ lut, AffM A, int G, int X, int Y,
                                                          int Z, int32_t* __restrict__ label, float* __restrict__ best) {
    const int sub = threadIdx.x / G, lane = threadIdx.x - sub * G, per = 256 / G;
    const int zb = per > 64 ? per : 64;
    const int j = blockIdx.y, k0 = blockIdx.x * zb;
    for (int i = blockIdx.z; i < X; i += gridDim.z) {
        for (int kk = sub; kk < zb; kk += per) {
            const int k = k0 + kk;                  // uniform over the G lanes of a voxel, and over a wave when G == 64
            if (k >= Z) break;
            const double x = affine_row(A, 0, i, j, k), y = affine_row(A, 1, i, j, k), z = affine_row(A, 2, i, j, k);
            const Foot F = foot_setup(x, y, z, D, H, W, C);
            float bv = 0.f;
            int bc = 0x7fffffff;
            if (F.any)
                for (int c = lane; c < C; c += G) {
                    const float v = foot_lerp(F, post + c);
                    if (v > bv) { bv = v; bc = c; }
                }
            for (int o = G >> 1; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oc = __shfl_xor(bc, o, 64);
                if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
            }
            if (lane == 0) {
                const int64_t o = ((int64_t)i * Y + j) * Z + k;
                label[o] = bc == 0x7fffffff ? 0 : lut[bc];
                if (best) best[o] = bv;
            }
        }
    }
}

inline bool load_m(const double* M, AffM& A) {
    for (int q = 0; q < 12; ++q) {
        A.m[q] = M[q];
        if (!(M[q] - M[q] == 0.0)) return false;            // NaN or infinite
    }
    return true;
}

}  // namespace

extern "C" int bfm_affine_pull_route(int C) {
    if (C < 1) return BFM_E_ARG;
    int g = 1;
    while (5 * g < C && g < 16) g <<= 1;                    // measured: see the kernel's comment
    return g;
}

extern "C" int bfm_affine_pull_multi(const float* src, int64_t map_stride, int K, int D, int H, int W, const double* M_host,
                                     const int* mode_host, int X, int Y, int Z, float* out, bfm_stream_t stream) {
    if (!src || !out || !M_host || !mode_host || K < 1) return BFM_E_ARG;
    if (D < 1 || H < 1 || W < 1 || X < 1 || Y < 1 || Z < 1 || map_stride < (int64_t)D * H * W) return BFM_E_SHAPE;
    if (bfm_cdiv(Y, 4) > 65535) return BFM_E_SHAPE;
    AffM A;
    if (!load_m(M_host, A)) return BFM_E_ARG;
    for (int m = 0; m < K; ++m)
        if (mode_host[m] != 0 && mode_host[m] != 1) return BFM_E_ARG;
    const int64_t nvox = (int64_t)X * Y * Z;
    const dim3 grid(bfm_cdiv(Z, 64), bfm_cdiv(Y, 4), std::min(X, 65535));
    for (int m0 = 0; m0 < K; m0 += 64) {                    // one launch up to 64 maps (the mode mask is one 64-bit word)
        const int kn = std::min(64, K - m0);
        uint64_t mask = 0;
        for (int m = 0; m < kn; ++m) mask |= (uint64_t)mode_host[m0 + m] << m;
        hipLaunchKernelGGL(affine_pull_multi, grid, dim3(64, 4), 0, bfm_s(stream), src + m0 * map_stride, map_stride, kn, D,
                           H, W, A, mask, X, Y, Z, out + m0 * nvox);
    }
    return bfm_launch_status();
}

extern "C" int bfm_affine_pull_argmax(const float* post, int C, int D, int H, int W, const int32_t* lut,
                                      const double* M_host, int X, int Y, int Z, int lanes, int32_t* label,
                                      float* best, bfm_stream_t stream) {
    if (!post || !lut || !M_host || !label || C < 1) return BFM_E_ARG;
    if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) return BFM_E_ARG;
    if (D < 1 || H < 1 || W < 1 || X < 1 || Y < 1 || Z < 1 || Y > 65535) return BFM_E_SHAPE;
    AffM A;
    if (!load_m(M_host, A)) return BFM_E_ARG;
    const int G = lanes ? lanes : bfm_affine_pull_route(C);
    hipLaunchKernelGGL(affine_pull_argmax, dim3(bfm_cdiv(Z, std::max(64, 256 / G)), Y, std::min(X, 65535)), dim3(256), 0,
                       bfm_s(stream), post, C, D, H, W, lut, A, G, X, Y, Z, label, best);
    return bfm_launch_status();
}
