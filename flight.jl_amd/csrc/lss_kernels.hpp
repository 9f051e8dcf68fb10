// lss_kernels.hpp — Model(lss): a batch of LinearizedSS models stepped on the device (FP/linearization.jl:157-192).
//   xdot = xdot0 + A (x - x0) + B (u - u0),   y = y0 + C (x - x0) + D (u - u0)
// One system per group of G lanes (G = 4, 8, 16 or 32, the smallest >= nx; 64 / G systems per wave, a group never straddles a wave);
// lane r of a group owns state row r. Lanes r >= nx and columns c >= nx are padding: their matrix entries, xdot0 and x0 are exact zeros in
// the handle's copy of the model, so their dx stays 0 and contributes a * 0 = 0.
//
// The layout of the handle's copy of the model (written by k_lss_gather only) is stated once, at fbg::ab_index and fbg::cd_index
// (lss_group.hpp), and read and written through them. State, inputs, outputs and derivative are the C ABI's rows: x [nx x n], u [nu x n], y [ny x n], xdot [nx x n].
//
// Exchange of the G stage values: fbg::Exchange<G, XCH> (lss_group.hpp), both instantiated; FLIGHTBATCH_LSS_EXCHANGE selects at create time.
#pragma once
#include "lss_group.hpp"

namespace fbl {

using fbg::Exchange;

constexpr int LSS_BLOCK = 256;
constexpr int LSS_NX_MAX = 32, LSS_NU_MAX = 8, LSS_NY_MAX = 64;

struct LssArgs {
    const double* ab; const double* xs; const double* u0; const double* y0; const double* cd;
    double* x; const double* u; double* y; double* xdot;
    int64_t n;
    int nx, nu, ny;
    double dt;
};

// the constant of a launch: xdot0_r + sum_c B_rc (u_c - u0_c), c ascending (u is held over the launch)
template <int G>
__device__ inline double lss_const(const LssArgs& a, int64_t i, int64_t slot) {
    const int64_t S = a.n * G;
    double c0 = a.xs[slot];
    for (int c = 0; c < a.nu; c++) c0 = fma(a.ab[fbg::ab_index(S, slot, G + c)], a.u[(int64_t)c * a.n + i] - a.u0[(int64_t)c * a.n + i], c0);
    return c0;
}

// nsteps of the classical RK4 in the stage form of the other steppers (robot2d_kernels.hpp: k_r2_step)
template <int G, int XCH>
__global__ __launch_bounds__(LSS_BLOCK) void k_lss_rk4(LssArgs a, int nsteps) {
    __shared__ __attribute__((aligned(16))) double panel[XCH == 0 ? LSS_BLOCK : 2];
    const int r = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * (LSS_BLOCK / G) + threadIdx.x / G;
    if (i >= a.n) return;   // (whole groups leave together; nothing below is a workgroup barrier)
    const int64_t S = a.n * G, slot = i * G + r;
    double arow[G];
#pragma unroll
    for (int c = 0; c < G; c++) arow[c] = a.ab[fbg::ab_index(S, slot, c)];
    const double x0 = a.xs[S + slot], c0 = lss_const<G>(a, i, slot);
    const bool live = r < a.nx;
    double x = live ? a.x[(int64_t)r * a.n + i] : 0.0;
    const double dt = a.dt, hdt = a.dt / 2, dt6 = a.dt / 6;
    const Exchange<G, XCH> ex(panel);
#pragma unroll 1
    for (int k = 0; k < nsteps; k++) {
        const double k1 = ex.dot(arow, x - x0, c0);
        const double k2 = ex.dot(arow, (x + hdt * k1) - x0, c0);
        const double k3 = ex.dot(arow, (x + hdt * k2) - x0, c0);
        const double k4 = ex.dot(arow, (x + dt * k3) - x0, c0);
        x = x + dt6 * (2 * (k2 + k3) + (k1 + k4));
    }
    if (live) a.x[(int64_t)r * a.n + i] = x;
}

// f_ode!(mdl): xdot (may be null) and y at the current x, u. A's row and C | D are streamed once.
template <int G>
__global__ __launch_bounds__(LSS_BLOCK) void k_lss_f_ode(LssArgs a) {
    __shared__ __attribute__((aligned(16))) double panel[LSS_BLOCK];
    const int r = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * (LSS_BLOCK / G) + threadIdx.x / G;
    if (i >= a.n) return;
    const int64_t S = a.n * G, slot = i * G + r;
    const bool live = r < a.nx;
    const double x = live ? a.x[(int64_t)r * a.n + i] : 0.0;
    double arow[G];
#pragma unroll
    for (int c = 0; c < G; c++) arow[c] = a.ab[fbg::ab_index(S, slot, c)];
    const Exchange<G, 0> ex(panel);
    const double xd = ex.dot(arow, x - a.xs[S + slot], lss_const<G>(a, i, slot));   // (the stepper's own expression: same bits as its k1)
    if (live && a.xdot) a.xdot[(int64_t)r * a.n + i] = xd;
    const double* dx = ex.row;   // the group's dx, left in the panel by dot()
    for (int j = r; j < a.ny; j += G) {
        double acc = a.y0[(int64_t)j * a.n + i];
        for (int c = 0; c < a.nx; c++) acc = fma(a.cd[fbg::cd_index(a.n, i, a.ny, j, c)], dx[c], acc);
        for (int c = 0; c < a.nu; c++)
            acc = fma(a.cd[fbg::cd_index(a.n, i, a.ny, j, a.nx + c)], a.u[(int64_t)c * a.n + i] - a.u0[(int64_t)c * a.n + i], acc);
        a.y[(int64_t)j * a.n + i] = acc;
    }
}

// subsystem(lss; x, u, y) device to device (FP/linearization.jl:113-132): the handle's copy of the model from a linearisation result in the
// layout fb_linearize writes (include/flightbatch.h): xdot0, x0 [snx x n], u0 [snu x n], y0 [sny x n], AB [(r + snx c) n + i] over the
// snx + snu columns of [A | B], CD [(j + sny c) n + i]. idx = ix[nx] | iu[nu] | iy[ny] (checked on the host against snx, snu, sny).
// Also Modeling.X(lss) = copy(x0), Modeling.U(lss) = copy(u0) (:157-158). One thread per system.
struct LssSrc {
    const double *xdot0, *x0, *u0, *y0, *AB, *CD;
    int snx, snu, sny;
    const int32_t* idx;
};
struct LssDst {
    double *ab, *xs, *u0, *y0, *cd, *x, *u;
    int nx, nu, ny, G;
    int64_t n;
};
__global__ __launch_bounds__(LSS_BLOCK) void k_lss_gather(LssSrc s, LssDst d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = d.n;
    if (i >= n) return;
    const int G = d.G;
    const int64_t S = n * G;
    const int32_t *ix = s.idx, *iu = ix + d.nx, *iy = iu + d.nu;
    for (int r = 0; r < G; r++) {
        const int64_t slot = i * G + r;
        const bool live = r < d.nx;
        const int sr = live ? ix[r] : 0;
        d.xs[slot] = live ? s.xdot0[(int64_t)sr * n + i] : 0.0;
        const double x0 = live ? s.x0[(int64_t)sr * n + i] : 0.0;
        d.xs[S + slot] = x0;
        if (live) d.x[(int64_t)r * n + i] = x0;
        for (int c = 0; c < G; c++)
            d.ab[fbg::ab_index(S, slot, c)] = (live && c < d.nx) ? s.AB[fbg::staged_index(n, i, s.snx, sr, ix[c])] : 0.0;
        for (int c = 0; c < d.nu; c++)
            d.ab[fbg::ab_index(S, slot, G + c)] = live ? s.AB[fbg::staged_index(n, i, s.snx, sr, s.snx + iu[c])] : 0.0;
    }
    for (int c = 0; c < d.nu; c++) {
        const double u0 = s.u0[(int64_t)iu[c] * n + i];
        d.u0[(int64_t)c * n + i] = u0;
        d.u[(int64_t)c * n + i] = u0;
    }
    for (int j = 0; j < d.ny; j++) {
        const int sj = iy[j];
        d.y0[(int64_t)j * n + i] = s.y0[(int64_t)sj * n + i];
        for (int c = 0; c < d.nx + d.nu; c++) {
            const int sc = c < d.nx ? ix[c] : s.snx + iu[c - d.nx];
            d.cd[fbg::cd_index(n, i, d.ny, j, c)] = s.CD[fbg::staged_index(n, i, s.sny, sj, sc)];
        }
    }
}

}  // namespace fbl

// The stepper of a sampled model (fb_lss_c2d; docs/design/linearize.md, "Sampled models on the device"): the handle's copy holds Phi in A's
// place, Gamma in B's and delta in xdot0's, and a step is the map itself,
//   x+ = x0 + Phi (x - x0) + Gamma (u - u0) + delta,
// one exchange where k_lss_rk4 takes four. Groups, exchanges and arguments are k_lss_rk4's; row r of Phi stays in registers with the
// launch constant delta_r + sum_c Gamma_rc (u_c - u0_c), and the step loop touches no global memory. (Its own namespace: fbl::k_lss_* is
// the set of the continuous model's instances.)
namespace fbz {

template <int G, int XCH>
__global__ __launch_bounds__(fbl::LSS_BLOCK) void k_lss_map(fbl::LssArgs a, int nsteps) {
    __shared__ __attribute__((aligned(16))) double panel[XCH == 0 ? fbl::LSS_BLOCK : 2];
    const int r = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * (fbl::LSS_BLOCK / G) + threadIdx.x / G;
    if (i >= a.n) return;   // (whole groups leave together; nothing below is a workgroup barrier)
    const int64_t S = a.n * G, slot = i * G + r;
    double prow[G];
#pragma unroll
    for (int c = 0; c < G; c++) prow[c] = a.ab[fbg::ab_index(S, slot, c)];
    const double x0 = a.xs[S + slot], c0 = fbl::lss_const<G>(a, i, slot);
    const bool live = r < a.nx;
    double x = live ? a.x[(int64_t)r * a.n + i] : 0.0;
    const fbg::Exchange<G, XCH> ex(panel);
#pragma unroll 1
    for (int k = 0; k < nsteps; k++) x = x0 + ex.dot(prow, x - x0, c0);
    if (live) a.x[(int64_t)r * a.n + i] = x;
}

}  // namespace fbz
