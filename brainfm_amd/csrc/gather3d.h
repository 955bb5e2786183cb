// Device pieces of fast_3D_interp_torch (Generator/utils.py:140-192) shared by every trilinear gather of the library:
// the texel load policy, the validity test, the corners and weights, and the lerp chain.  Built with -ffp-contract=off:
// a*b + c*d stays mul, mul, add like the reference's eager torch ops.
#pragma once
#include "bfm_common.h"

// Texel loads of the gathers (data-dependent addresses, lines re-used from the L1 by neighbouring lanes and waves) go past
// the per-CU vector L1: agent scope = global_load_dword sc1, served by the XCD's L2.  Round 3 cornered what round 2 had
// only worked around (HISTORY.md section 3.3, tests/diag/diag_atlas_repro.py, profiles/r03_atlas_gather_hazard.txt): with
// ordinary loads such a gather gets wrong texels -- whole 16-lane groups -- whenever a kernel that fills its LDS by LDS-DMA
// (global_load_lds, every conv kernel here) runs beside it on another stream; an L1 invalidate at kernel start does not
// help, L1-bypassing loads (agent or system scope) do.  The value type is float or a 4-byte bit pattern.
__device__ __forceinline__ float ld_tex(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_tex(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The same policy for wider texels: a buffer descriptor over the volume (num_records = its bytes, so a load past the end
// returns 0 instead of touching memory) and loads with aux 16 = sc1, i.e. L1-bypassing like ld_tex.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tex_rsrc(const float* X, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X), 0, bytes, 0x00020000);
}
typedef int v3i_t __attribute__((ext_vector_type(3)));
// three consecutive floats (one channels-last voxel of a 3-channel field) at byte offset `off`
__device__ __forceinline__ void ld_tex3(__amdgpu_buffer_rsrc_t R, uint32_t off, float& a, float& b, float& c) {
    const v3i_t v = __builtin_amdgcn_raw_buffer_load_b96(R, off, 0, 16);
    a = __int_as_float(v.x); b = __int_as_float(v.y); c = __int_as_float(v.z);
}

// :141, ok: strict lower bound, inclusive upper bound
__device__ __forceinline__ bool interp_ok(float x, float y, float z, int nx, int ny, int nz) {
    return (x > 0.f) && (y > 0.f) && (z > 0.f) && (x <= (float)(nx - 1)) && (y <= (float)(ny - 1)) &&
           (z <= (float)(nz - 1));
}

// :147-163 for a valid sample: floor, the upper corner clamped to n-1, wc = I - floor(I), wf = 1 - wc
struct Trilin {
    int fx, fy, fz, cx, cy, cz;
    float wcx, wcy, wcz, wfx, wfy, wfz;
};
__device__ __forceinline__ Trilin trilin_setup(float x, float y, float z, int nx, int ny, int nz) {
    Trilin t;
    const float fxf = floorf(x), fyf = floorf(y), fzf = floorf(z);
    t.fx = (int)fxf; t.fy = (int)fyf; t.fz = (int)fzf;
    t.cx = min(t.fx + 1, nx - 1); t.cy = min(t.fy + 1, ny - 1); t.cz = min(t.fz + 1, nz - 1);
    t.wcx = x - fxf; t.wcy = y - fyf; t.wcz = z - fzf;
    t.wfx = 1.f - t.wcx; t.wfy = 1.f - t.wcy; t.wfz = 1.f - t.wcz;
    return t;
}

// :177-185, the c00 ... c chain; texel tXYZ is the corner (X ? cx : fx, Y ? cy : fy, Z ? cz : fz)
__device__ __forceinline__ float trilin_lerp(const Trilin& t, float t000, float t100, float t010, float t110, float t001,
                                             float t101, float t011, float t111) {
    const float c00 = t000 * t.wfx + t100 * t.wcx;
    const float c01 = t001 * t.wfx + t101 * t.wcx;
    const float c10 = t010 * t.wfx + t110 * t.wcx;
    const float c11 = t011 * t.wfx + t111 * t.wcx;
    const float c0 = c00 * t.wfy + c10 * t.wcy;
    const float c1 = c01 * t.wfy + c11 * t.wcy;
    return c0 * t.wfz + c1 * t.wcz;
}

// fast_3D_interp_torch(X, x, y, z, 'linear') of a 3-channel channels-last volume [nx][ny][nz][3] (R over its bytes): the
// eight corners are one 12-byte load each; 0 where not ok (default_value_linear = 0).  SCALE: the volume is m * X (every
// texel multiplied by m before the lerp, as if m * X had been materialised first).
template <bool SCALE>
__device__ __forceinline__ void interp3_c3(__amdgpu_buffer_rsrc_t R, int nx, int ny, int nz, float x, float y, float z,
                                           float m, float r[3]) {
    r[0] = 0.f; r[1] = 0.f; r[2] = 0.f;
    if (!interp_ok(x, y, z, nx, ny, nz)) return;
    const Trilin t = trilin_setup(x, y, z, nx, ny, nz);
    const uint32_t sx = (uint32_t)ny * nz * 12u, sy = (uint32_t)nz * 12u;
    float a[8][3];
    ld_tex3(R, t.fx * sx + t.fy * sy + t.fz * 12u, a[0][0], a[0][1], a[0][2]);
    ld_tex3(R, t.cx * sx + t.fy * sy + t.fz * 12u, a[1][0], a[1][1], a[1][2]);
    ld_tex3(R, t.fx * sx + t.cy * sy + t.fz * 12u, a[2][0], a[2][1], a[2][2]);
    ld_tex3(R, t.cx * sx + t.cy * sy + t.fz * 12u, a[3][0], a[3][1], a[3][2]);
    ld_tex3(R, t.fx * sx + t.fy * sy + t.cz * 12u, a[4][0], a[4][1], a[4][2]);
    ld_tex3(R, t.cx * sx + t.fy * sy + t.cz * 12u, a[5][0], a[5][1], a[5][2]);
    ld_tex3(R, t.fx * sx + t.cy * sy + t.cz * 12u, a[6][0], a[6][1], a[6][2]);
    ld_tex3(R, t.cx * sx + t.cy * sy + t.cz * 12u, a[7][0], a[7][1], a[7][2]);
    if constexpr (SCALE) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { a[k][0] = a[k][0] * m; a[k][1] = a[k][1] * m; a[k][2] = a[k][2] * m; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        r[c] = trilin_lerp(t, a[0][c], a[1][c], a[2][c], a[3][c], a[4][c], a[5][c], a[6][c], a[7][c]);
}
