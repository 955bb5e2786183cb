// Dormand-Prince integration of the advection PDE with the step controller ON the device
// (ShapeID/DiffEqs/dopri5.py:58-172, rk_common.py:22-61, misc.py:145-170, interp.py:5-65; RHS: pde.py:616-640).
//
// Round 1-3: every stage was two launches (rk_combine, advect_rhs), every step ended in a host read-back of the error
// norm and host arithmetic for accept / reject / next step (13 launches + 1 sync per step, Python-bound).  Here
//   * a stage is ONE kernel: the stage state y + dt * sum_j beta_ij k_j is evaluated at the 7 stencil points straight
//     from y and the k_j (the same expressions as rk_combine, so the same bits) -- the stage state is never written;
//   * the error norm, accept / reject, the clamped next step (dopri5.py:150-169) and the dense output at the requested
//     times are computed by kernels that read and update a small state block in device memory;
//   * the host enqueues steps in chunks and reads back one flag per chunk; kernels of steps past the end exit at once.
// The state keeps y0's dtype (fp64 for Perlin shapes, fp32 for file maps) with fp32 stages, like the reference.
// The right-hand side of a stage is box_rhs<T, CFG> below: the generator's upwind advection (CFG_ADV), or the diffusion
// terms and the general velocity of pde.py:362-441, :511-524, chosen at compile time.
#include "bfm_common.h"

#include <type_traits>

namespace {

inline int grid_for(int64_t n, int tpb = 256, int cap = 8192) {
    int64_t b = bfm_cdiv64(n, tpb);
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

struct OdeState {
    double t0s, t1s, dt, step_dt;      // last accepted interval, next step size, size of the step just taken
    double msr;                        // mean squared error ratio of the step just taken
    int cur, done, next_out, nsteps, naccept, accepted, err, pad;
};

// The fields of the diffusion term and of the general-velocity term (pde.py:362-441, :511-524).  D: {D} for a scalar field,
// {Dxx, Dyy, Dzz, Dxy, Dyz, Dxz} for a tensor; G: the time-invariant central differences of D that multiply c_x C, c_y C,
// c_z C (pde_central_sum below); divV = c_x Vx + c_y Vy + c_z Vz.
struct PdeTerms { const float* D[6]; const float* G[3]; const float* divV; float Dc; };

struct OdeArgs {
    void* y[2]; float* f[2]; float* k[5];
    const float *Vx, *Vy, *Vz;
    int sx, sy, sz, neumann;
    OdeState* st;
    PdeTerms P;
};

__constant__ double BETA[6][6] = {
    {1 / 5., 0, 0, 0, 0, 0},
    {3 / 40., 9 / 40., 0, 0, 0, 0},
    {44 / 45., -56 / 15., 32 / 9., 0, 0, 0},
    {19372 / 6561., -25360 / 2187., 64448 / 6561., -212 / 729., 0, 0},
    {9017 / 3168., -355 / 33., 46732 / 5247., 49 / 176., -5103 / 18656., 0},
    {35 / 384., 0, 500 / 1113., 125 / 192., -2187 / 6784., 11 / 84.}};
__constant__ double C_ERR[7] = {35 / 384. - 1951 / 21600., 0, 500 / 1113. - 22642 / 50085., 125 / 192. - 451 / 720.,
                                -2187 / 6784. - -12231 / 42400., 11 / 84. - 649 / 6300., -1. / 60.};
__constant__ double C_MID[7] = {6025192743 / 30085553152. / 2, 0, 51252292925 / 65400821598. / 2,
                                -2691868925 / 45128329728. / 2, 187940372067 / 1594534317056. / 2,
                                -1776094331 / 19743644256. / 2, 11237099 / 235043384. / 2};

// (dt * c) in the state dtype, then the fp32 value torch's 0-dim promotion multiplies the fp32 stage with (misc.py:22-25)
template <typename T>
__device__ __forceinline__ float coef(double dt, double c) { return (float)((T)dt * (T)c); }

// k_STAGE = f(y + dt * sum_{j < STAGE} beta[STAGE-1][j] k_j).  A workgroup owns an 8 x 8 x 32 box of voxels: the stage
// state of the box and its one-voxel halo (10 x 10 x 34 points) is evaluated once into LDS -- the expression of rk_combine
// at the boundary-conditioned position, so the same bits --, then every thread forms the upwind RHS of its 8 voxels from
// LDS.  The stage state never goes to HBM; the k_j are read 1.66x (the halo) instead of 7x (one evaluation per stencil
// point, first form of this kernel: 415 us per step against 283 for the separate rk_combine + advect_rhs launches).
// STAGE 6 also stores y1 (the UNconditioned combination) and f1, and leaves the block partials of the error norm
// (rk_error_partial's expression: err = sum_j c_j k_j with k_6 = the value just computed).
constexpr int TX = 8, TY = 8, TZ = 32;
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;

// ---- the right-hand side of one voxel from the boundary-conditioned state of its box in LDS -------------------------
// CFG = VK + 4 * DK selects the terms at compile time: VK 0 no advection, 1 upwind advection by a divergence-free V
// (Grad_div_free_vectorV), 2 by a general V (Grad_vectorV: minus C div V);  DK 0 no diffusion, 1 constant, 2 scalar,
// 3 diagonal, 4 full tensor (Grad_constantD .. Grad_fullD).  CFG_ADV is the configuration of the generator and takes
// none of the other code.  With f / b / c the forward / backward / central differences of pde.py:13-190 (one-sided at
// the ends, every difference taken in the state dtype and rounded to fp32 as gradient_* stores it), a term reads the
// 3 x 3 x 3 neighbourhood of its voxel, except b_a(f_a C) at index 0 of axis a, which is f_a[1] - f_a[0] and reads
// index 2: inside the box of any volume with 3 voxels per axis.  At the last index b_a(f_a C) is f_a[n-1] - f_a[n-2]
// with both equal to C[n-1] - C[n-2]: exactly 0.
constexpr int V_NONE = 0, V_DIVFREE = 1, V_GENERAL = 2;
constexpr int D_NONE = 0, D_CONSTANT = 1, D_SCALAR = 2, D_DIAG = 3, D_FULL = 4;
constexpr int CFG_ADV = V_DIVFREE + 4 * D_NONE;

// the reference's result dtype: C * div V promotes to the state dtype (pde.py:524); every other term is fp32
template <typename T, int CFG>
using rhs_t = std::conditional_t<(CFG & 3) == V_GENERAL, T, float>;

template <typename T, int CFG>
__device__ __forceinline__ rhs_t<T, CFG> box_rhs(const T* __restrict__ sU, int tx, int ty, int tz, int x, int yy, int z,
                                                 int sx, int sy, int sz, int64_t i, const float* __restrict__ Vx,
                                                 const float* __restrict__ Vy, const float* __restrict__ Vz,
                                                 const PdeTerms& P) {
    constexpr int VK = CFG & 3, DK = CFG >> 2;
    auto U = [&](int dx, int dy, int dz) -> T { return sU[((tx + 1 + dx) * HY + (ty + 1 + dy)) * HZ + (tz + 1 + dz)]; };
    const T u = U(0, 0, 0);
    float kv = 0.f;
    if constexpr (VK != V_NONE) {
        float acc = 0.f;
        bool first = true;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const int pos = ax == 0 ? x : (ax == 1 ? yy : z);
            const int len = ax == 0 ? sx : (ax == 1 ? sy : sz);
            const int ex = ax == 0, ey = ax == 1, ez = ax == 2;
            const int fw = pos < len - 1 ? 1 : 0, bw = pos > 0 ? 1 : 0;
            const T up = U(ex * fw, ey * fw, ez * fw);
            const T dn = U(-ex * bw, -ey * bw, -ez * bw);
            const float df = pos < len - 1 ? (float)(up - u) : (float)(u - dn);
            const float db = pos > 0 ? (float)(u - dn) : (float)(up - u);
            const float V = ax == 0 ? Vx[i] : (ax == 1 ? Vy[i] : Vz[i]);
            const float flag = V > 0.f ? 1.f : 0.f;
            const float d = df * (1.f - flag) + db * flag;
            const float term = V * d;
            acc = first ? term : acc + term;
            first = false;
        }
        kv = -acc;
    }
    if constexpr (CFG == CFG_ADV) {
        return kv;
    } else {
        float kd = 0.f;
        if constexpr (DK != D_NONE) {
            const int pos[3] = {x, yy, z}, len[3] = {sx, sy, sz};
            // b_a(f_a C)
            auto dd = [&](int a) -> float {
                const int e0 = a == 0, e1 = a == 1, e2 = a == 2;
                if (pos[a] == len[a] - 1) return 0.f;
                const float f1 = (float)(U(e0, e1, e2) - u);
                if (pos[a] == 0) return (float)(U(2 * e0, 2 * e1, 2 * e2) - U(e0, e1, e2)) - f1;
                return f1 - (float)(u - U(-e0, -e1, -e2));
            };
            // c_a C
            auto dc = [&](int a) -> float {
                const int e0 = a == 0, e1 = a == 1, e2 = a == 2;
                if (pos[a] == 0) return (float)(U(e0, e1, e2) - u);
                if (pos[a] == len[a] - 1) return (float)(u - U(-e0, -e1, -e2));
                return (float)((U(e0, e1, e2) - U(-e0, -e1, -e2)) / (T)2);
            };
            // b_a(f_g C), a != g: f_g at the voxel and at its neighbour along a (an edge neighbour of the halo)
            auto cr = [&](int a, int g) -> float {
                const int a0 = a == 0, a1 = a == 1, a2 = a == 2, g0 = g == 0, g1 = g == 1, g2 = g == 2;
                const bool fwd = pos[g] < len[g] - 1;
                auto fg = [&](int s) -> float {
                    const T c0 = U(s * a0, s * a1, s * a2);
                    return fwd ? (float)(U(s * a0 + g0, s * a1 + g1, s * a2 + g2) - c0)
                               : (float)(c0 - U(s * a0 - g0, s * a1 - g1, s * a2 - g2));
                };
                return pos[a] > 0 ? fg(0) - fg(-1) : fg(1) - fg(0);
            };
            if constexpr (DK == D_CONSTANT) {
                kd = P.Dc * ((dd(0) + dd(1)) + dd(2));
            } else if constexpr (DK == D_SCALAR) {
                const float D = P.D[0][i];
                kd = (P.G[0][i] * dc(0) + P.G[1][i] * dc(1)) + P.G[2][i] * dc(2);
                kd = kd + D * dd(0);
                kd = kd + D * dd(1);
                kd = kd + D * dd(2);
            } else if constexpr (DK == D_DIAG) {
                kd = P.G[0][i] * dc(0) + P.D[0][i] * dd(0);
                kd = kd + P.G[1][i] * dc(1);
                kd = kd + P.D[1][i] * dd(1);
                kd = kd + P.G[2][i] * dc(2);
                kd = kd + P.D[2][i] * dd(2);
            } else {
                kd = P.G[0][i] * dc(0) + P.G[1][i] * dc(1);
                kd = kd + P.G[2][i] * dc(2);
                kd = kd + P.D[0][i] * dd(0);
                kd = kd + P.D[1][i] * dd(1);
                kd = kd + P.D[2][i] * dd(2);
                kd = kd + P.D[3][i] * (cr(0, 1) + cr(1, 0));
                kd = kd + P.D[4][i] * (cr(1, 2) + cr(2, 1));
                kd = kd + P.D[5][i] * (cr(2, 0) + cr(0, 2));
            }
        }
        if constexpr (VK == V_GENERAL) {
            T r = (T)kv - u * (T)P.divV[i];
            if constexpr (DK != D_NONE) r = r + (T)kd;
            return r;
        } else if constexpr (VK == V_DIVFREE) {
            return kv + kd;
        } else {
            return kd;
        }
    }
}

template <typename T, int STAGE, int CFG>
__global__ void __launch_bounds__(256) ode_stage(OdeArgs A, double atol, double rtol, double* __restrict__ part) {
    const OdeState* st = A.st;
    if (st->done) return;
    __shared__ T sU[HX * HY * HZ];
    __shared__ float sE[STAGE == 6 ? TX * TY * TZ : 1];             // stage 6: sum_{j<6} c_err[j] k_j at the box's voxels
    const int cur = st->cur;
    const T* __restrict__ y = static_cast<const T*>(A.y[cur]);
    const float* ks[6] = {A.f[cur], A.k[0], A.k[1], A.k[2], A.k[3], A.k[4]};
    float* __restrict__ out = STAGE == 6 ? A.f[cur ^ 1] : A.k[STAGE - 1];
    T* __restrict__ ynext = static_cast<T*>(A.y[cur ^ 1]);
    float c[STAGE];
#pragma unroll
    for (int j = 0; j < STAGE; ++j) c[j] = coef<T>(st->dt, BETA[STAGE - 1][j]);
    float ce[7];
    if (STAGE == 6) {
#pragma unroll
        for (int j = 0; j < 7; ++j) ce[j] = coef<T>(st->dt, C_ERR[j]);
    }
    const int sx = A.sx, sy = A.sy, sz = A.sz;
    const int64_t stx = (int64_t)sy * sz, sty = sz;
    const int nbz = (sz + TZ - 1) / TZ, nby = (sy + TY - 1) / TY;
    const int bz = blockIdx.x % nbz, by = (blockIdx.x / nbz) % nby, bx = blockIdx.x / (nbz * nby);
    const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZ;
    // ---- phase 1: the stage state on the box + halo
    for (int p = threadIdx.x; p < HX * HY * HZ; p += 256) {
        const int hz = p % HZ, hy = (p / HZ) % HY, hx = p / (HZ * HY);
        int a = x0 + hx - 1, b = y0 + hy - 1, cc = z0 + hz - 1;
        if (A.neumann) {
            a = min(max(a, 1), sx - 2); b = min(max(b, 1), sy - 2); cc = min(max(cc, 1), sz - 2);
        } else {
            a = min(max(a, 0), sx - 1); b = min(max(b, 0), sy - 1); cc = min(max(cc, 0), sz - 1);   // never used beyond the faces
        }
        const int64_t q = a * stx + b * sty + cc;
        float kv[STAGE];
#pragma unroll
        for (int j = 0; j < STAGE; ++j) kv[j] = ks[j][q];
        float acc = c[0] * kv[0];
#pragma unroll
        for (int j = 1; j < STAGE; ++j) acc = acc + c[j] * kv[j];
        sU[p] = (T)(y[q] + (T)acc);
        if (STAGE == 6 && hx >= 1 && hx <= TX && hy >= 1 && hy <= TY && hz >= 1 && hz <= TZ) {
            // interior point of the halo box: q is the voxel itself unless a Neumann face moved it (those are redone below)
            float e = ce[0] * kv[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) e = e + ce[j] * kv[j];
            sE[((hx - 1) * TY + (hy - 1)) * TZ + (hz - 1)] = e;
        }
    }
    __syncthreads();
    // ---- phase 2: upwind right-hand side of the box's voxels
    const int tz = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int yy = y0 + ty, z = z0 + tz;
    double es = 0.0;
    if (yy < sy && z < sz) {
#pragma unroll 2
        for (int tx = 0; tx < TX; ++tx) {
            const int x = x0 + tx;
            if (x >= sx) break;
            const int64_t i = x * stx + yy * sty + z;
            const T u = sU[((tx + 1) * HY + (ty + 1)) * HZ + (tz + 1)];
            const auto rk = box_rhs<T, CFG>(sU, tx, ty, tz, x, yy, z, sx, sy, sz, i, A.Vx, A.Vy, A.Vz, A.P);
            const float kn = (float)rk;
            out[i] = kn;
            if (STAGE == 6) {
                // y1 is the UNconditioned combination at i (rk_combine); the LDS value is boundary-conditioned, which
                // differs on the faces under Neumann conditions
                const bool face = A.neumann && (x == 0 || x == sx - 1 || yy == 0 || yy == sy - 1 || z == 0 || z == sz - 1);
                T y1v = u;
                if (face) {
                    float a6 = c[0] * ks[0][i];
#pragma unroll
                    for (int j = 1; j < STAGE; ++j) a6 = a6 + c[j] * ks[j][i];
                    y1v = (T)(y[i] + (T)a6);
                }
                ynext[i] = y1v;
                float e = sE[(tx * TY + ty) * TZ + tz];
                if (face) {
                    e = ce[0] * ks[0][i];
#pragma unroll
                    for (int j = 1; j < 6; ++j) e = e + ce[j] * ks[j][i];
                }
                e = e + ce[6] * kn;
                const T tol = (T)atol + (T)rtol * (T)fmax((double)fabs((double)y[i]), (double)fabs((double)y1v));
                const T r = (T)e / tol;
                es += (double)(r * r);
            }
        }
    }
    if (STAGE == 6) {
        __shared__ double red[4];
        es = wave_reduce_sum(es);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = es;
        __syncthreads();
        if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

struct CtlP { double tol_min_dt, dt_max, safety, ifactor, dfactor; int64_t n; };

// one block: fold the boxes' partials of the error norm (fixed order), then _optimal_step_size + the forced-accept clamps of
// dopri5.py:150-169 on thread 0
__global__ void ode_control(OdeState* st, const double* __restrict__ part, int nb, CtlP P) {
    if (st->done) return;
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) s += part[i];
    s = wave_reduce_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double total = (red[0] + red[1]) + (red[2] + red[3]);
    const double msr = total / (double)P.n;
    const double dt = st->dt;
    if (!(st->t1s + dt > st->t1s)) { st->err = 1; st->done = 1; return; }       // 'underflow in dt'
    const bool accept = msr <= 1;
    double dt_next;
    if (msr == 0) {
        dt_next = dt * P.ifactor;
    } else {
        const double dfactor = msr < 1 ? 1.0 : P.dfactor;
        // Python's min / max keep their first argument unless the second compares smaller / larger: a NaN error norm
        // (a diverged state) gives factor = 1 / ifactor there, and must here
        const double a = pow(sqrt(msr), 1.0 / 5.0) / P.safety, b = 1 / dfactor;
        const double inner = b < a ? b : a;
        const double factor = inner > 1 / P.ifactor ? inner : 1 / P.ifactor;
        dt_next = dt / factor;
    }
    bool advance;
    if (!(dt_next < P.tol_min_dt || dt_next > P.dt_max)) {
        advance = accept;
    } else {
        dt_next = dt_next < P.tol_min_dt ? P.tol_min_dt : dt_next;
        dt_next = dt_next > P.dt_max ? P.dt_max : dt_next;
        advance = true;
    }
    st->msr = msr;
    st->accepted = advance ? 1 : 0;
    if (advance) {
        st->step_dt = dt;
        st->t0s = st->t1s;
        st->t1s = st->t1s + dt;
        st->cur ^= 1;
        st->naccept += 1;
    }
    st->dt = dt_next;
    st->nsteps += 1;
}

// _interp_fit_dopri5 + _interp_evaluate (dopri5.py:41-47, interp.py:5-65) at every requested time inside the interval just
// accepted; the expressions of dense_eval (synth_shape.hip)
template <typename T>
__global__ void ode_dense(OdeArgs A, const double* __restrict__ t_out, int nt, T* __restrict__ sol, int64_t n) {
    const OdeState* st = A.st;
    if (st->done || !st->accepted) return;
    const int cur = st->cur;                                            // already the NEW state
    const T* __restrict__ y0 = static_cast<const T*>(A.y[cur ^ 1]);
    const T* __restrict__ y1 = static_cast<const T*>(A.y[cur]);
    const float* ks[7] = {A.f[cur ^ 1], A.k[0], A.k[1], A.k[2], A.k[3], A.k[4], A.f[cur]};
    const double t0 = st->t0s, t1 = st->t1s;
    const T dt = (T)st->step_dt;
    float cm[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) cm[j] = coef<T>(st->step_dt, C_MID[j]);
    for (int o = st->next_out; o < nt && t_out[o] <= t1; ++o) {
        const T x = (T)(((T)t_out[o] - (T)t0) / ((T)t1 - (T)t0));
        const T x2 = x * x, x3 = x2 * x, x4 = x3 * x;
        T* __restrict__ dst = sol + (int64_t)o * n;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            float m = cm[0] * ks[0][i];
#pragma unroll
            for (int j = 1; j < 7; ++j) m = m + cm[j] * ks[j][i];
            const T a0 = y0[i], a1 = y1[i];
            const T ym = a0 + (T)m;
            const float f0 = ks[0][i], f1 = ks[6][i];
            const T ca = ((((T)((float)(-2 * dt) * f0 + (float)(2 * dt) * f1)) + (T)(-8) * a0) + (T)(-8) * a1) + (T)16 * ym;
            const T cb = ((((T)((float)(5 * dt) * f0 + (float)(-3 * dt) * f1)) + (T)18 * a0) + (T)14 * a1) + (T)(-32) * ym;
            const T cc = ((((T)((float)(-4 * dt) * f0 + (float)dt * f1)) + (T)(-11) * a0) + (T)(-5) * a1) + (T)16 * ym;
            const float cd = (float)dt * f0;
            dst[i] = (((ca * x4 + cb * x3) + cc * x2) + (T)(cd * (float)x)) + a0 * (T)1;
        }
    }
}

// after the dense outputs of a step: move next_out past the interval; the last requested time ends the integration
__global__ void ode_after_dense(OdeState* st, const double* __restrict__ t_out, int nt) {
    if (st->done || !st->accepted) return;
    int o = st->next_out;
    while (o < nt && t_out[o] <= st->t1s) ++o;
    st->next_out = o;
    st->accepted = 0;
    if (o >= nt) st->done = 1;
}

__global__ void ode_init(OdeState* st, double t0, double dt0) {
    st->t0s = t0; st->t1s = t0; st->dt = dt0; st->step_dt = 0; st->msr = 0;
    st->cur = 0; st->done = 0; st->next_out = 1; st->nsteps = 0; st->naccept = 0; st->accepted = 0; st->err = 0; st->pad = 0;
}


// CFG of a terms block (NULL: the generator's 'adv' with a divergence-free V), -1 if it names no built configuration or
// lacks a field that configuration reads
int pde_cfg(const bfm_pde_terms_t* t, const float* Vx, const float* Vy, const float* Vz) {
    const bool hasV = Vx && Vy && Vz;
    if (!t) return hasV ? CFG_ADV : -1;
    const bool adv = t->perf & BFM_PDE_ADV, diff = t->perf & BFM_PDE_DIFF;
    if ((!adv && !diff) || (t->perf & ~(BFM_PDE_ADV | BFM_PDE_DIFF))) return -1;
    int vk = V_NONE, dk = D_NONE;
    if (adv) {
        if (!hasV || (t->v_general && !t->divV)) return -1;
        vk = t->v_general ? V_GENERAL : V_DIVFREE;
    }
    if (diff) {
        dk = t->d_type;
        if (dk < D_CONSTANT || dk > D_FULL) return -1;
        const int nd = dk == D_CONSTANT ? 0 : (dk == D_SCALAR ? 1 : (dk == D_DIAG ? 3 : 6));
        for (int j = 0; j < nd; ++j) if (!t->D[j]) return -1;
        if (dk != D_CONSTANT) for (int j = 0; j < 3; ++j) if (!t->G[j]) return -1;
    }
    return vk + 4 * dk;
}

PdeTerms pde_terms(const bfm_pde_terms_t* t) {
    PdeTerms P{};
    if (!t) return P;
    for (int j = 0; j < 6; ++j) P.D[j] = t->D[j];
    for (int j = 0; j < 3; ++j) P.G[j] = t->G[j];
    P.divV = t->divV; P.Dc = t->D_const;
    return P;
}

// f(std::integral_constant<int, CFG>) for the built configuration `cfg`
template <typename F>
bool pde_dispatch(int cfg, F&& f) {
    switch (cfg) {
#define BFM_PDE_CASE(VK, DK) case (VK) + 4 * (DK): f(std::integral_constant<int, (VK) + 4 * (DK)>{}); return true;
        BFM_PDE_CASE(V_DIVFREE, D_NONE) BFM_PDE_CASE(V_GENERAL, D_NONE)
        BFM_PDE_CASE(V_NONE, D_CONSTANT) BFM_PDE_CASE(V_DIVFREE, D_CONSTANT) BFM_PDE_CASE(V_GENERAL, D_CONSTANT)
        BFM_PDE_CASE(V_NONE, D_SCALAR) BFM_PDE_CASE(V_DIVFREE, D_SCALAR) BFM_PDE_CASE(V_GENERAL, D_SCALAR)
        BFM_PDE_CASE(V_NONE, D_DIAG) BFM_PDE_CASE(V_DIVFREE, D_DIAG) BFM_PDE_CASE(V_GENERAL, D_DIAG)
        BFM_PDE_CASE(V_NONE, D_FULL) BFM_PDE_CASE(V_DIVFREE, D_FULL) BFM_PDE_CASE(V_GENERAL, D_FULL)
#undef BFM_PDE_CASE
        default: return false;
    }
}

bool ode_ok(const bfm_dopri5_advect_t* d, const bfm_pde_terms_t* t) {
    if (!d || !d->y[0] || !d->y[1] || !d->f[0] || !d->f[1] || !d->state || !d->workspace || !d->t_out || !d->sol ||
        d->nt < 2 || pde_cfg(t, d->Vx, d->Vy, d->Vz) < 0)
        return false;
    for (int j = 0; j < 5; ++j) if (!d->k[j]) return false;
    return d->sx >= 3 && d->sy >= 3 && d->sz >= 3 && (int64_t)d->sx * d->sy <= INT32_MAX;
}

OdeArgs ode_args(const bfm_dopri5_advect_t* d, const bfm_pde_terms_t* t) {
    OdeArgs A;
    A.P = pde_terms(t);
    A.y[0] = d->y[0]; A.y[1] = d->y[1]; A.f[0] = d->f[0]; A.f[1] = d->f[1];
    for (int j = 0; j < 5; ++j) A.k[j] = d->k[j];
    A.Vx = d->Vx; A.Vy = d->Vy; A.Vz = d->Vz;
    A.sx = d->sx; A.sy = d->sy; A.sz = d->sz; A.neumann = d->neumann_bc ? 1 : 0;
    A.st = static_cast<OdeState*>(d->state);
    return A;
}

int ode_boxes(const bfm_dopri5_advect_t* d) {
    return ((d->sx + TX - 1) / TX) * ((d->sy + TY - 1) / TY) * ((d->sz + TZ - 1) / TZ);
}

template <typename T, int CFG>
void ode_enqueue_step(const bfm_dopri5_advect_t* d, const OdeArgs& A, hipStream_t s) {
    const int64_t n = (int64_t)d->sx * d->sy * d->sz;
    const int nb = ode_boxes(d);
    const dim3 gs(nb), bs(256);
    double* part = static_cast<double*>(d->workspace);
    hipLaunchKernelGGL((ode_stage<T, 1, CFG>), gs, bs, 0, s, A, d->atol, d->rtol, part);
    hipLaunchKernelGGL((ode_stage<T, 2, CFG>), gs, bs, 0, s, A, d->atol, d->rtol, part);
    hipLaunchKernelGGL((ode_stage<T, 3, CFG>), gs, bs, 0, s, A, d->atol, d->rtol, part);
    hipLaunchKernelGGL((ode_stage<T, 4, CFG>), gs, bs, 0, s, A, d->atol, d->rtol, part);
    hipLaunchKernelGGL((ode_stage<T, 5, CFG>), gs, bs, 0, s, A, d->atol, d->rtol, part);
    hipLaunchKernelGGL((ode_stage<T, 6, CFG>), gs, bs, 0, s, A, d->atol, d->rtol, part);
    CtlP P{d->tol_min_dt, d->dt_max, d->safety, d->ifactor, d->dfactor, n};
    hipLaunchKernelGGL(ode_control, dim3(1), bs, 0, s, A.st, part, nb, P);
    hipLaunchKernelGGL(ode_dense<T>, dim3(grid_for(n)), bs, 0, s, A, d->t_out, d->nt, static_cast<T*>(d->sol), n);
    hipLaunchKernelGGL(ode_after_dense, dim3(1), dim3(1), 0, s, A.st, d->t_out, d->nt);
}

}  // namespace

extern "C" size_t bfm_dopri5_advect_state_bytes(void) { return sizeof(OdeState); }
extern "C" size_t bfm_dopri5_advect_workspace(int sx, int sy, int sz) {
    return (size_t)((sx + TX - 1) / TX) * ((sy + TY - 1) / TY) * ((sz + TZ - 1) / TZ) * sizeof(double);
}

extern "C" int bfm_dopri5_advdiff_init(const bfm_dopri5_advect_t* d, const bfm_pde_terms_t* terms, double t0, double dt0,
                                       bfm_stream_t stream) {
    if (!ode_ok(d, terms) || !(dt0 > 0)) return BFM_E_ARG;
    hipLaunchKernelGGL(ode_init, dim3(1), dim3(1), 0, bfm_s(stream), static_cast<OdeState*>(d->state), t0, dt0);
    return bfm_launch_status();
}

extern "C" int bfm_dopri5_advdiff_steps(const bfm_dopri5_advect_t* d, const bfm_pde_terms_t* terms, int nsteps,
                                        bfm_stream_t stream) {
    if (!ode_ok(d, terms) || nsteps <= 0) return BFM_E_ARG;
    const OdeArgs A = ode_args(d, terms);
    pde_dispatch(pde_cfg(terms, d->Vx, d->Vy, d->Vz), [&](auto cfg) {
        constexpr int CFG = decltype(cfg)::value;
        for (int s = 0; s < nsteps; ++s) {
            if (d->is_f64) ode_enqueue_step<double, CFG>(d, A, bfm_s(stream));
            else ode_enqueue_step<float, CFG>(d, A, bfm_s(stream));
        }
    });
    return bfm_launch_status();
}

extern "C" int bfm_dopri5_advect_init(const bfm_dopri5_advect_t* d, double t0, double dt0, bfm_stream_t stream) {
    return bfm_dopri5_advdiff_init(d, nullptr, t0, dt0, stream);
}

extern "C" int bfm_dopri5_advect_steps(const bfm_dopri5_advect_t* d, int nsteps, bfm_stream_t stream) {
    return bfm_dopri5_advdiff_steps(d, nullptr, nsteps, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Fixed-grid solvers: euler, midpoint, rk4 (DiffEqs/fixed_grid.py:5-33, solvers.py:158-207, rk_common.py:72-78).
// The grid is the requested times, so step i reads row i of the (nt, ...) solution and writes row i + 1: no controller,
// no state block, no read-back; the whole integration is enqueued at once.  A stage is the box kernel of ode_stage
// above: stage state y + sum_j c_j k_j on the box and its halo into LDS (rk_combine's expression at the
// boundary-conditioned position), then the upwind RHS from LDS.  The LAST stage of a step does not store its k: the
// thread that formed k_n at voxel i also forms y1[i] = y[i] + (sum_{j < NF} cf_j k_j[i] + cf_NF k_n), rk_combine's
// expression over (k_1 .. k_n) at the UNconditioned position, and stores it into the next row.
//   NK: stages in the stage state (0: the state itself);  NF: earlier stages in the final sum, -1: not the last stage.
// The coefficients come from the host already rounded to the fp32 values the unfused route hands to rk_combine.
namespace {

struct FixedArgs {
    const float* k[3]; float c[3]; float cf[4];
    const float *Vx, *Vy, *Vz;
    float* kout;
    int sx, sy, sz, neumann;
    PdeTerms P;
    double* kout64;     // a general V with an fp64 state, stand-alone RHS only: the unrounded value (pde.py:524 promotes)
};

template <typename T, int NK, int NF, int CFG>
__global__ void __launch_bounds__(256) ode_fixed_stage(const T* __restrict__ y, T* __restrict__ y1, FixedArgs A) {
    __shared__ T sU[HX * HY * HZ];
    const int sx = A.sx, sy = A.sy, sz = A.sz;
    const int64_t stx = (int64_t)sy * sz, sty = sz;
    const int nbz = (sz + TZ - 1) / TZ, nby = (sy + TY - 1) / TY;
    const int bz = blockIdx.x % nbz, by = (blockIdx.x / nbz) % nby, bx = blockIdx.x / (nbz * nby);
    const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZ;
    // ---- phase 1: the stage state on the box + halo
    for (int p = threadIdx.x; p < HX * HY * HZ; p += 256) {
        const int hz = p % HZ, hy = (p / HZ) % HY, hx = p / (HZ * HY);
        int a = x0 + hx - 1, b = y0 + hy - 1, cc = z0 + hz - 1;
        if (A.neumann) {
            a = min(max(a, 1), sx - 2); b = min(max(b, 1), sy - 2); cc = min(max(cc, 1), sz - 2);
        } else {
            a = min(max(a, 0), sx - 1); b = min(max(b, 0), sy - 1); cc = min(max(cc, 0), sz - 1);   // never used beyond the faces
        }
        const int64_t q = a * stx + b * sty + cc;
        T v = y[q];
        if (NK > 0) {
            float acc = A.c[0] * A.k[0][q];
#pragma unroll
            for (int j = 1; j < NK; ++j) acc = acc + A.c[j] * A.k[j][q];
            v = (T)(v + (T)acc);
        }
        sU[p] = v;
    }
    __syncthreads();
    // ---- phase 2: upwind right-hand side of the box's voxels
    const int tz = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int yy = y0 + ty, z = z0 + tz;
    if (yy < sy && z < sz) {
#pragma unroll 2
        for (int tx = 0; tx < TX; ++tx) {
            const int x = x0 + tx;
            if (x >= sx) break;
            const int64_t i = x * stx + yy * sty + z;
            const auto rk = box_rhs<T, CFG>(sU, tx, ty, tz, x, yy, z, sx, sy, sz, i, A.Vx, A.Vy, A.Vz, A.P);
            const float kn = (float)rk;
            if constexpr (NF < 0) {
                if constexpr (std::is_same<rhs_t<T, CFG>, double>::value) {
                    if (A.kout64) A.kout64[i] = rk;
                    else A.kout[i] = kn;
                } else {
                    A.kout[i] = kn;
                }
            } else if constexpr (NF == 0) {
                y1[i] = (T)(y[i] + (T)(A.cf[0] * kn));
            } else {
                float s = A.cf[0] * A.k[0][i];
#pragma unroll
                for (int j = 1; j < NF; ++j) s = s + A.cf[j] * A.k[j][i];
                s = s + A.cf[NF] * kn;
                y1[i] = (T)(y[i] + (T)s);
            }
        }
    }
}

template <typename T, int NK, int NF, int CFG>
void fixed_launch(const T* y, T* y1, const FixedArgs& A, int nb, hipStream_t s) {
    hipLaunchKernelGGL((ode_fixed_stage<T, NK, NF, CFG>), dim3(nb), dim3(256), 0, s, y, y1, A);
}

template <typename T, int CFG>
void fixed_enqueue(const bfm_ode_fixed_advect_t* d, const bfm_pde_terms_t* t, hipStream_t s) {
    const int64_t n = (int64_t)d->sx * d->sy * d->sz;
    const int nb = ((d->sx + TX - 1) / TX) * ((d->sy + TY - 1) / TY) * ((d->sz + TZ - 1) / TZ);
    FixedArgs A{};
    A.P = pde_terms(t);
    A.Vx = d->Vx; A.Vy = d->Vy; A.Vz = d->Vz;
    A.sx = d->sx; A.sy = d->sy; A.sz = d->sz; A.neumann = d->neumann_bc ? 1 : 0;
    for (int j = 0; j < 3; ++j) A.k[j] = d->k[j];
    T* sol = static_cast<T*>(d->sol);
    for (int i = 0; i + 1 < d->nt; ++i) {
        const T* y = sol + (int64_t)i * n;
        T* y1 = sol + (int64_t)(i + 1) * n;
        const float* c = d->coef + (size_t)i * bfm_ode_fixed_ncoef(d->method);
        if (d->method == BFM_ODE_EULER) {                       // dy = dt * f(y)
            A.cf[0] = c[0];
            fixed_launch<T, 0, 0, CFG>(y, y1, A, nb, s);
        } else if (d->method == BFM_ODE_MIDPOINT) {             // dy = dt * f(y + f(y) * dt / 2)
            A.kout = d->k[0];
            fixed_launch<T, 0, -1, CFG>(y, y1, A, nb, s);
            A.c[0] = c[0]; A.cf[0] = c[1];
            fixed_launch<T, 1, 0, CFG>(y, y1, A, nb, s);
        } else {                                                // the 3/8 rule, rk4_alt_step_func
            A.kout = d->k[0];
            fixed_launch<T, 0, -1, CFG>(y, y1, A, nb, s);
            A.c[0] = c[0]; A.kout = d->k[1];
            fixed_launch<T, 1, -1, CFG>(y, y1, A, nb, s);
            A.c[0] = c[1]; A.c[1] = c[2]; A.kout = d->k[2];
            fixed_launch<T, 2, -1, CFG>(y, y1, A, nb, s);
            A.c[0] = c[3]; A.c[1] = c[4]; A.c[2] = c[5];
            A.cf[0] = c[6]; A.cf[1] = c[7]; A.cf[2] = c[8]; A.cf[3] = c[9];
            A.kout = nullptr;
            fixed_launch<T, 3, 3, CFG>(y, y1, A, nb, s);
        }
    }
}

}  // namespace

extern "C" int bfm_ode_fixed_ncoef(int method) {
    return method == BFM_ODE_EULER ? 1 : (method == BFM_ODE_MIDPOINT ? 2 : (method == BFM_ODE_RK4 ? 10 : 0));
}

extern "C" int bfm_ode_fixed_advdiff(const bfm_ode_fixed_advect_t* d, const bfm_pde_terms_t* terms, bfm_stream_t stream) {
    if (!d || !d->sol || !d->coef || d->nt < 2) return BFM_E_ARG;
    const int cfg = pde_cfg(terms, d->Vx, d->Vy, d->Vz);
    if (cfg < 0) return BFM_E_ARG;
    const int nk = d->method == BFM_ODE_EULER ? 0 : (d->method == BFM_ODE_MIDPOINT ? 1 : (d->method == BFM_ODE_RK4 ? 3 : -1));
    if (nk < 0) return BFM_E_ARG;
    for (int j = 0; j < nk; ++j) if (!d->k[j]) return BFM_E_ARG;
    if (d->sx < 3 || d->sy < 3 || d->sz < 3 || (int64_t)d->sx * d->sy > INT32_MAX) return BFM_E_ARG;
    pde_dispatch(cfg, [&](auto c) {
        constexpr int CFG = decltype(c)::value;
        if (d->is_f64) fixed_enqueue<double, CFG>(d, terms, bfm_s(stream));
        else fixed_enqueue<float, CFG>(d, terms, bfm_s(stream));
    });
    return bfm_launch_status();
}

extern "C" int bfm_ode_fixed_advect(const bfm_ode_fixed_advect_t* d, bfm_stream_t stream) {
    return bfm_ode_fixed_advdiff(d, nullptr, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The stand-alone right-hand side (AdvDiffPDE.forward and the unfused host routes): the first stage of the fixed-grid
// kernel, k_1 = f(y), so the bits of the fused routes.  Derived fields: sums of central differences of fp32 fields.
namespace {

// out = sum_j c_{axis[j]}(f[j]), j < nterms, added left to right in fp32 (gradient_c of pde.py:127-186)
struct CentralSum { const float* f[3]; int axis[3]; int nterms; };

__global__ void pde_central_sum(CentralSum S, int sx, int sy, int sz, float* __restrict__ out) {
    const int64_t n = (int64_t)sx * sy * sz;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % sz), y = (int)((i / sz) % sy), x = (int)(i / ((int64_t)sz * sy));
        float acc = 0.f;
        for (int j = 0; j < S.nterms; ++j) {
            const int a = S.axis[j];
            const int pos = a == 0 ? x : (a == 1 ? y : z), len = a == 0 ? sx : (a == 1 ? sy : sz);
            const int64_t st = a == 0 ? (int64_t)sy * sz : (a == 1 ? sz : 1);
            const float* __restrict__ f = S.f[j];
            float d;
            if (pos == 0) d = f[i + st] - f[i];
            else if (pos == len - 1) d = f[i] - f[i - st];
            else d = (f[i + st] - f[i - st]) / 2.f;
            acc = j == 0 ? d : acc + d;
        }
        out[i] = acc;
    }
}

}  // namespace

extern "C" int bfm_pde_central_sum(const float* const* f, const int* axis, int nterms, int sx, int sy, int sz, float* out,
                                   bfm_stream_t stream) {
    if (!f || !axis || !out || nterms < 1 || nterms > 3 || sx < 2 || sy < 2 || sz < 2) return BFM_E_ARG;
    CentralSum S{};
    S.nterms = nterms;
    for (int j = 0; j < nterms; ++j) {
        if (!f[j] || axis[j] < 0 || axis[j] > 2) return BFM_E_ARG;
        S.f[j] = f[j]; S.axis[j] = axis[j];
    }
    const int64_t n = (int64_t)sx * sy * sz;
    hipLaunchKernelGGL(pde_central_sum, dim3(grid_for(n)), dim3(256), 0, bfm_s(stream), S, sx, sy, sz, out);
    return bfm_launch_status();
}

extern "C" int bfm_advdiff_rhs(const void* C, int c_is_f64, const float* Vx, const float* Vy, const float* Vz,
                               const bfm_pde_terms_t* terms, int sx, int sy, int sz, int neumann_bc, void* out,
                               int out_is_f64, bfm_stream_t stream) {
    if (!C || !out) return BFM_E_ARG;
    const int cfg = pde_cfg(terms, Vx, Vy, Vz);
    if (cfg < 0) return BFM_E_ARG;
    if (sx < 3 || sy < 3 || sz < 3 || (int64_t)sx * sy > INT32_MAX) return BFM_E_ARG;
    if (out_is_f64 && !(c_is_f64 && (cfg & 3) == V_GENERAL)) return BFM_E_ARG;     // only that product promotes
    FixedArgs A{};
    A.P = pde_terms(terms);
    A.Vx = Vx; A.Vy = Vy; A.Vz = Vz;
    A.sx = sx; A.sy = sy; A.sz = sz; A.neumann = neumann_bc ? 1 : 0;
    if (out_is_f64) A.kout64 = static_cast<double*>(out);
    else A.kout = static_cast<float*>(out);
    const int nb = ((sx + TX - 1) / TX) * ((sy + TY - 1) / TY) * ((sz + TZ - 1) / TZ);
    pde_dispatch(cfg, [&](auto c) {
        constexpr int CFG = decltype(c)::value;
        if (c_is_f64) fixed_launch<double, 0, -1, CFG>(static_cast<const double*>(C), nullptr, A, nb, bfm_s(stream));
        else fixed_launch<float, 0, -1, CFG>(static_cast<const float*>(C), nullptr, A, nb, bfm_s(stream));
    });
    return bfm_launch_status();
}
