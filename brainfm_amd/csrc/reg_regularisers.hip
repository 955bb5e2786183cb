// Regularisers of the predicted MNI coordinates: SmoothnessLoss('l2') and HessianLoss('l2') of
// Trainer/models/losses.py:72-130, applied by criterion.py:187-191 to outputs['registration'] -- the raw head output, no
// processor -- with their gradients w.r.t. that output ADDED (times coef) into the registration columns of dRaw.
//
//   D_a u      forward difference along axis a (x = W, y = H, z = D), zero on the last index of that axis
//   smooth     mean_{c,v} sum_a (D_a u)^2            gradient (2 / N) sum_a D_a^T D_a u,  N = nch * D * H * W
//   hessian    sum_{c,v} det(H)^2, H_ab = D_a D_b u  gradient sum_ab (D_a D_b)^T [2 det ddet/dH_ab]
//   D^T g [i] = g[i-1] [i >= 1] - g[i] [i < n-1]     (the adjoint of the zeroed forward difference)
//
// Element (c, v) of the field sits at base[col_offset + c * chan_stride + v * voxel_stride]: rows of voxels
// (chan_stride = row pitch, voxel_stride 1) or channels-last (chan_stride 1, voxel_stride n_out); dRaw has the same layout.
// Loss sums are fp64 per-block partials folded in a fixed order: no atomics, the same bits on every run.  Differences,
// the Hessian and its determinant are formed in fp64 from the fp32 field (first and second differences of fp32 values are
// exact there); the Hessian's per-voxel cofactor terms are kept in LDS as fp32.
//
// The Hessian kernel works on an LDS tile with a halo instead of two passes through a scratch buffer: the gradient at p
// needs the cofactor terms at p and at up to two voxels below it on each axis, and those need u up to two voxels above
// them.  One block stages u over tile + 2 on both sides, forms det and the six terms over tile + 2 below, and applies
// the adjoints: about 60 bytes of HBM traffic per voxel and channel less than a pass that writes and re-reads the six
// terms, and no scratch field (300 MB at 160^3).
#include "bfm_common.h"

namespace {

constexpr int NT = 256;
constexpr int SM_BLOCKS = 1024;                      // partial blocks of the smoothness reduction

// Hessian tile: TX x TY x TZ output voxels of one channel per block
constexpr int TX = 32, TY = 4, TZ = 4;
constexpr int UX = TX + 4, UY = TY + 4, UZ = TZ + 4;  // u over [origin - 2, end + 2)
constexpr int GX = TX + 2, GY = TY + 2, GZ = TZ + 2;  // det terms over [origin - 2, end)
constexpr int NU = UX * UY * UZ, NG = GX * GY * GZ, NO = TX * TY * TZ;

__device__ __forceinline__ double block_sum(double v, double* red) {          // NT threads, fixed tree
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(NT) fold_kernel(const double* __restrict__ part, int nb, double scale,
                                                  double* __restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += NT) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s * scale;
}

// One thread per voxel, every channel; the six neighbours come from L1 / L2.
__global__ void __launch_bounds__(NT) smooth_kernel(const float* __restrict__ raw, int64_t off, int64_t cs, int64_t vs,
                                                    int nch, int D, int H, int W, double gcoef, float* __restrict__ dRaw,
                                                    double* __restrict__ part) {
    __shared__ double red[NT];
    const int64_t nvox = (int64_t)D * H * W, HW = (int64_t)H * W;
    double acc = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * NT + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * NT) {
        const int x = (int)(v % W);
        const int y = (int)((v / W) % H);
        const int z = (int)(v / HW);
        for (int c = 0; c < nch; ++c) {
            const float* u = raw + off + c * cs;
            const double u0 = u[v * vs];
            double g = 0.0;                                   // sum_a D_a^T D_a u at v
            if (x < W - 1) { const double d = (double)u[(v + 1) * vs] - u0; acc += d * d; g -= d; }
            if (x > 0) g += u0 - (double)u[(v - 1) * vs];
            if (y < H - 1) { const double d = (double)u[(v + W) * vs] - u0; acc += d * d; g -= d; }
            if (y > 0) g += u0 - (double)u[(v - W) * vs];
            if (z < D - 1) { const double d = (double)u[(v + HW) * vs] - u0; acc += d * d; g -= d; }
            if (z > 0) g += u0 - (double)u[(v - HW) * vs];
            if (dRaw) dRaw[off + c * cs + v * vs] += (float)(gcoef * g);
        }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// grid (tiles_x, tiles_y, tiles_z * nch); block = one channel's TX x TY x TZ tile
__global__ void __launch_bounds__(NT) hessian_kernel(const float* __restrict__ raw, int64_t off, int64_t cs, int64_t vs,
                                                     int D, int H, int W, int tiles_z, float coef,
                                                     float* __restrict__ dRaw, double* __restrict__ part) {
    __shared__ float su[NU];
    __shared__ float sg[6][NG];                          // 2 det ddet/dH_ab: xx yy zz xy xz yz
    __shared__ double red[NT];
    const int c = blockIdx.z / tiles_z;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = (blockIdx.z - c * tiles_z) * TZ;
    const int64_t HW = (int64_t)H * W;
    const float* u = raw + off + c * cs;

    for (int i = threadIdx.x; i < NU; i += NT) {
        const int lx = i % UX, ly = (i / UX) % UY, lz = i / (UX * UY);
        const int gx = x0 - 2 + lx, gy = y0 - 2 + ly, gz = z0 - 2 + lz;
        float val = 0.f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H && gz >= 0 && gz < D) val = u[((int64_t)gz * HW + (int64_t)gy * W + gx) * vs];
        su[i] = val;
    }
    __syncthreads();

    double acc = 0.0;
    for (int i = threadIdx.x; i < NG; i += NT) {
        const int lx = i % GX, ly = (i / GX) % GY, lz = i / (GX * GY);
        const int qx = x0 - 2 + lx, qy = y0 - 2 + ly, qz = z0 - 2 + lz;
        double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (qx >= 0 && qx < W && qy >= 0 && qy < H && qz >= 0 && qz < D) {
            const int b = (lz * UY + ly) * UX + lx;          // q in the u region (same origin)
            const int ex = 1, ey = UX, ez = UX * UY;
            const double u0 = su[b];
            const double ux = su[b + ex], uxx = su[b + 2 * ex];
            const double uy = su[b + ey], uyy = su[b + 2 * ey];
            const double uz = su[b + ez], uzz = su[b + 2 * ez];
            const double uxy = su[b + ex + ey], uxz = su[b + ex + ez], uyz = su[b + ey + ez];
            const bool mx = qx < W - 1, my = qy < H - 1, mz = qz < D - 1;
            // D_a D_a u = [i < n-1] ((D_a u)[i+1] - (D_a u)[i]),  (D_a u)[i+1] zero at i + 1 = n - 1
            const double xx = mx ? ((qx < W - 2 ? uxx - ux : 0.0) - (ux - u0)) : 0.0;
            const double yy = my ? ((qy < H - 2 ? uyy - uy : 0.0) - (uy - u0)) : 0.0;
            const double zz = mz ? ((qz < D - 2 ? uzz - uz : 0.0) - (uz - u0)) : 0.0;
            const double xy = (mx && my) ? (uxy - ux - uy + u0) : 0.0;
            const double xz = (mx && mz) ? (uxz - ux - uz + u0) : 0.0;
            const double yz = (my && mz) ? (uyz - uy - uz + u0) : 0.0;
            const double det = xx * (yy * zz - yz * yz) - xy * (xy * zz - xz * yz) + xz * (xy * yz - xz * yy);
            if (lx >= 2 && ly >= 2 && lz >= 2) acc += det * det;     // q is one of this block's own voxels
            const double d2 = 2.0 * det;
            t[0] = d2 * (yy * zz - yz * yz);
            t[1] = d2 * (xx * zz - xz * xz);
            t[2] = d2 * (xx * yy - xy * xy);
            t[3] = 2.0 * d2 * (xz * yz - xy * zz);
            t[4] = 2.0 * d2 * (xy * yz - xz * yy);
            t[5] = 2.0 * d2 * (xy * xz - xx * yz);
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) sg[a][i] = (float)t[a];
    }
    acc = block_sum(acc, red);                          // also the barrier between the terms and their adjoints
    if (threadIdx.x == 0) part[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
    if (!dRaw) return;

    for (int i = threadIdx.x; i < NO; i += NT) {
        const int ox = i % TX, oy = (i / TX) % TY, oz = i / (TX * TY);
        const int px = x0 + ox, py = y0 + oy, pz = z0 + oz;
        if (px >= W || py >= H || pz >= D) continue;
        const int b = ((oz + 2) * GY + (oy + 2)) * GX + (ox + 2);   // p in the term region
        const int ex = 1, ey = GX, ez = GX * GY;
        const bool lx1 = px >= 1, lx2 = px >= 2, hx = px < W - 1;
        const bool ly1 = py >= 1, ly2 = py >= 2, hy = py < H - 1;
        const bool lz1 = pz >= 1, lz2 = pz >= 2, hz = pz < D - 1;
        double r = 0.0;
        // (D_a D_a)^T g [i] = [i>=1] ([i>=2] g[i-2] - g[i-1]) - [i<n-1] ([i>=1] g[i-1] - g[i])
        {
            const float* g = sg[0];
            r += (lx1 ? ((lx2 ? (double)g[b - 2 * ex] : 0.0) - g[b - ex]) : 0.0) - (hx ? ((lx1 ? (double)g[b - ex] : 0.0) - g[b]) : 0.0);
            g = sg[1];
            r += (ly1 ? ((ly2 ? (double)g[b - 2 * ey] : 0.0) - g[b - ey]) : 0.0) - (hy ? ((ly1 ? (double)g[b - ey] : 0.0) - g[b]) : 0.0);
            g = sg[2];
            r += (lz1 ? ((lz2 ? (double)g[b - 2 * ez] : 0.0) - g[b - ez]) : 0.0) - (hz ? ((lz1 ? (double)g[b - ez] : 0.0) - g[b]) : 0.0);
        }
        // (D_a D_b)^T g = [i>=1][j>=1] g[i-1,j-1] - [i>=1][j<nb-1] g[i-1,j] - [i<na-1][j>=1] g[i,j-1] + [i<na-1][j<nb-1] g[i,j]
        {
            const float* g = sg[3];
            r += (lx1 && ly1 ? (double)g[b - ex - ey] : 0.0) - (lx1 && hy ? (double)g[b - ex] : 0.0) -
                 (hx && ly1 ? (double)g[b - ey] : 0.0) + (hx && hy ? (double)g[b] : 0.0);
            g = sg[4];
            r += (lx1 && lz1 ? (double)g[b - ex - ez] : 0.0) - (lx1 && hz ? (double)g[b - ex] : 0.0) -
                 (hx && lz1 ? (double)g[b - ez] : 0.0) + (hx && hz ? (double)g[b] : 0.0);
            g = sg[5];
            r += (ly1 && lz1 ? (double)g[b - ey - ez] : 0.0) - (ly1 && hz ? (double)g[b - ey] : 0.0) -
                 (hy && lz1 ? (double)g[b - ez] : 0.0) + (hy && hz ? (double)g[b] : 0.0);
        }
        const int64_t v = (int64_t)pz * HW + (int64_t)py * W + px;
        dRaw[off + c * cs + v * vs] += (float)((double)coef * r);
    }
}

int hessian_blocks(int nch, int D, int H, int W) {
    return bfm_cdiv(W, TX) * bfm_cdiv(H, TY) * bfm_cdiv(D, TZ) * nch;
}

bool reg_args_ok(const float* raw, int64_t off, int64_t cs, int64_t vs, int nch, int D, int H, int W,
                 const double* loss_out, const void* workspace) {
    return raw && loss_out && workspace && off >= 0 && cs > 0 && vs > 0 && nch > 0 && D > 0 && H > 0 && W > 0 &&
           (reinterpret_cast<uintptr_t>(workspace) & 7) == 0;
}

}  // namespace

extern "C" size_t bfm_loss_reg_workspace(int nch, int D, int H, int W) {
    if (nch <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)std::max(SM_BLOCKS, hessian_blocks(nch, D, H, W)) * sizeof(double);
}

extern "C" int bfm_loss_reg_smooth(const float* raw, int64_t col_offset, int64_t chan_stride, int64_t voxel_stride, int nch,
                                   int D, int H, int W, float coef, float* dRaw, double* loss_out, void* workspace,
                                   size_t workspace_bytes, bfm_stream_t stream) {
    if (!reg_args_ok(raw, col_offset, chan_stride, voxel_stride, nch, D, H, W, loss_out, workspace)) return BFM_E_ARG;
    if (workspace_bytes < bfm_loss_reg_workspace(nch, D, H, W)) return BFM_E_WORKSPACE;
    const int64_t nvox = (int64_t)D * H * W;
    const double n = (double)nch * (double)nvox;
    const int nb = (int)std::min<int64_t>(SM_BLOCKS, bfm_cdiv64(nvox, NT));
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(smooth_kernel, dim3(nb), dim3(NT), 0, bfm_s(stream), raw, col_offset, chan_stride, voxel_stride, nch,
                       D, H, W, (double)coef * 2.0 / n, dRaw, part);
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(NT), 0, bfm_s(stream), part, nb, 1.0 / n, loss_out);
    return bfm_launch_status();
}

extern "C" int bfm_loss_reg_hessian(const float* raw, int64_t col_offset, int64_t chan_stride, int64_t voxel_stride, int nch,
                                    int D, int H, int W, float coef, float* dRaw, double* loss_out, void* workspace,
                                    size_t workspace_bytes, bfm_stream_t stream) {
    if (!reg_args_ok(raw, col_offset, chan_stride, voxel_stride, nch, D, H, W, loss_out, workspace)) return BFM_E_ARG;
    if (workspace_bytes < bfm_loss_reg_workspace(nch, D, H, W)) return BFM_E_WORKSPACE;
    const int tx = bfm_cdiv(W, TX), ty = bfm_cdiv(H, TY), tz = bfm_cdiv(D, TZ);
    if (ty > 65535 || (int64_t)tz * nch > 65535) return BFM_E_SHAPE;
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(hessian_kernel, dim3(tx, ty, tz * nch), dim3(NT), 0, bfm_s(stream), raw, col_offset, chan_stride,
                       voxel_stride, D, H, W, tz, coef, dRaw, part);
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(NT), 0, bfm_s(stream), part, hessian_blocks(nch, D, H, W), 1.0, loss_out);
    return bfm_launch_status();
}
