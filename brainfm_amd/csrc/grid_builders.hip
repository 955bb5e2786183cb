// interpol.identity_grid / add_identity_grid_ / affine_grid in 3-D (utils/interpol/api.py:455-560): the voxel-index grid is
// written, or added in place, from the thread's own index; no meshgrid exists.  The values are the reference's bit for bit
// in fp32 and fp64: an index is exact in either, add_identity_grid_ is one addition per component, and affine_grid is
// matvec(lin, idx) + off (utils.py:81-108) in its summation order, ((l0 * x + l1 * y) + l2 * z) + off, products and sums
// rounded one by one (the library is built with -ffp-contract=off).
#include "bfm_common.h"

namespace {

inline int grid_for(int64_t n, int tpb = 256, int cap = 8192) {
    int64_t b = bfm_cdiv64(n, tpb);
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// out (nb, nx, ny, nz, 3); mat (nb, 3, 4) row-major, or NULL for the identity
template <typename F>
__global__ void __launch_bounds__(256) affine_grid3d(const F* __restrict__ mat, int64_t nb, int nx, int ny, int nz,
                                                     F* __restrict__ out) {
    const int64_t nvox = (int64_t)nx * ny * nz, n = nb * nvox;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / nvox, v = i - b * nvox;
        const int z = (int)(v % nz), y = (int)((v / nz) % ny), x = (int)(v / ((int64_t)nz * ny));
        const F fx = (F)x, fy = (F)y, fz = (F)z;
        F* o = out + i * 3;
        if (!mat) {
            o[0] = fx; o[1] = fy; o[2] = fz;
            continue;
        }
        const F* m = mat + b * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = ((m[r * 4] * fx + m[r * 4 + 1] * fy) + m[r * 4 + 2] * fz) + m[r * 4 + 3];
    }
}

// disp (nb, nx, ny, nz, 3) += the voxel index
template <typename F>
__global__ void __launch_bounds__(256) add_identity3d(F* __restrict__ disp, int64_t nb, int nx, int ny, int nz) {
    const int64_t nvox = (int64_t)nx * ny * nz, n = nb * nvox;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = i % nvox;
        const int z = (int)(v % nz), y = (int)((v / nz) % ny), x = (int)(v / ((int64_t)nz * ny));
        F* o = disp + i * 3;
        o[0] += (F)x; o[1] += (F)y; o[2] += (F)z;
    }
}

}  // namespace

extern "C" int bfm_affine_grid3d(const void* mat, int is_f64, int64_t nb, int nx, int ny, int nz, void* out,
                                 bfm_stream_t stream) {
    if (!out || nb <= 0 || nx <= 0 || ny <= 0 || nz <= 0) return BFM_E_ARG;
    const int64_t n = nb * nx * ny * nz;
    if (is_f64)
        hipLaunchKernelGGL(affine_grid3d<double>, dim3(grid_for(n)), dim3(256), 0, bfm_s(stream),
                           static_cast<const double*>(mat), nb, nx, ny, nz, static_cast<double*>(out));
    else
        hipLaunchKernelGGL(affine_grid3d<float>, dim3(grid_for(n)), dim3(256), 0, bfm_s(stream),
                           static_cast<const float*>(mat), nb, nx, ny, nz, static_cast<float*>(out));
    return bfm_launch_status();
}

extern "C" int bfm_add_identity_grid3d(void* disp, int is_f64, int64_t nb, int nx, int ny, int nz, bfm_stream_t stream) {
    if (!disp || nb <= 0 || nx <= 0 || ny <= 0 || nz <= 0) return BFM_E_ARG;
    const int64_t n = nb * nx * ny * nz;
    if (is_f64)
        hipLaunchKernelGGL(add_identity3d<double>, dim3(grid_for(n)), dim3(256), 0, bfm_s(stream), static_cast<double*>(disp),
                           nb, nx, ny, nz);
    else
        hipLaunchKernelGGL(add_identity3d<float>, dim3(grid_for(n)), dim3(256), 0, bfm_s(stream), static_cast<float*>(disp),
                           nb, nx, ny, nz);
    return bfm_launch_status();
}
