// timeresp_kernels.hpp — step responses and StepInfo of a batch of linear models on the device (include/flightbatch.h: fb_lss_stepinfo;
// host side: fb_timeresp.inc; docs/design/linearize.md, "Step responses on the device"; numpy restatement, operation for operation:
// tests/timeresp_prototype.py). Reference: `step(P[:y, :u], t_sim)` and `stepinfo` of it, as FA design/robot2d/robot2d_design.ipynb calls them
// on the velocity loop and on the position loop, and design/c172/c172x_design.jl after every loop it closes.
//   channel   (iu, iy) of a Model(lss) system in deviation coordinates: x' = A x + b, y = c x + d, b = B[:, iu], c = C[iy, :], d = D[iy, iu],
//             from rest; samples t_k = k dt, k = 0 .. N, by the classical RK4 in the stage form of the other steppers
//   StepInfo  y0 = y_0 and yf = y_N unless the caller gives them, dir = sign(yf - y0), stepsize = |yf - y0|; peak = the extremum on dir's side
//             at its first index; overshoot = dir 100 (peak - yf) / stepsize; undershoot = 100 (y0 - min y) / stepsize (dir > 0), not below 0;
//             settling time = t one sample past the last with |y - yf| > th stepsize (clamped to t_N, 0 if none);
//             rise time = t[first dir (y - y0) > hi stepsize] - t[first dir (y - y0) > lo stepsize], NaN if either is never reached
// Differences from the reference: ControlSystems.step picks its own sample time and discretises exactly; here dt is the caller's and the
// integrator is RK4. The exact samples at the caller's dt: fb_lss_c2d, then the same call on the sampled handle (fbz::k_timeresp_map, below).
//
// k_timeresp: one (system, channel) pair per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx + 1; 64 / P pairs per wave, one
// wave per workgroup); pair q = j n + i, system fastest. Lanes 0 .. nx - 1 own the rows of A with the constant b_r, lane nx owns the output
// row c with the constant d: the broadcast dot product that is the first stage of step k is, on that lane, sample k (k_pid_metrics'
// arrangement; stage values travel through Exchange<P, 0>). yf is known only when the trajectory ends and N samples fit nowhere on chip, so
// the trajectory is run twice: pass 1 records the endpoints, the extrema and the blow-up flag and stores the samples asked for; pass 2 repeats
// the same recurrence (every product that could be fused is an explicit fma: the two loops cannot round differently) and records the
// two first crossings and the last sample outside the settling band. Lanes past the batch's end work on the last pair again and store
// nothing, so a wave never diverges on the batch size.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbt {

using namespace fbg;

constexpr int TR_WAVE = fbg::WAVE;
constexpr double TR_BLOWUP = 1e12;      // |y| beyond this: FB_STEPINFO_DIVERGED

struct TimeRespArgs {
    const double* ab; const double* cd;   // the handle's copies (fbg::ab_index, lss_group.hpp), G its group size
    const int32_t* iu; const int32_t* iy; // [m]
    const double* y0_in; const double* yf_in;   // null or [m x n]; NaN = the first / last sample
    double* y;                            // null or [ns x m x n]: sample s stride at row s, sample N at row ns - 1
    double* info;                         // [9 x m x n]
    int32_t* status;                      // [m x n]
    int64_t n;
    int nx, nu, ny, G, m, nsteps, stride, ns;
    double dt, settling_th, rise_lo, rise_hi;
};

template <int P>
__global__ __launch_bounds__(TR_WAVE) void k_timeresp(TimeRespArgs a) {
    __shared__ __attribute__((aligned(16))) double panel[TR_WAVE];
    const fbg::Lanes<P> g;
    constexpr int NG = TR_WAVE / P;
    const int r = g.r, nx = a.nx, N = a.nsteps;
    const int64_t total = a.n * a.m;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n, j = q / a.n;
    const int iu = a.iu[j], iy = a.iy[j];
    const int64_t S = a.n * a.G, slot0 = i * a.G;

    // this lane's row: of A, or the output row
    const bool state = r < nx, outlane = r == nx;
    double row[P];
#pragma unroll
    for (int c = 0; c < P; c++) {
        double v = 0.0;
        if (c < nx) {
            if (state) v = a.ab[ab_index(S, slot0, c) + r];
            else if (outlane) v = a.cd[cd_index(a.n, i, a.ny, iy, c)];
        }
        row[c] = v;
    }
    const double c0 = state ? a.ab[ab_index(S, slot0, a.G + iu) + r] : outlane ? a.cd[cd_index(a.n, i, a.ny, iy, nx + iu)] : 0.0;

    const double dt = a.dt, hdt = a.dt / 2, dt6 = a.dt / 6;
    const fbg::Exchange<P, 0> ex(panel);

    // ---- pass 1: endpoints, extrema at their first index, blow-up; the samples asked for
    double first = 0.0, last = 0.0, mx = -__builtin_inf(), mn = __builtin_inf();
    int imx = 0, imn = 0;
    bool blown = false;
    {
        const bool store = a.y != nullptr && valid && outlane;
        int64_t at = q;
        int next = 0;
        double x = 0.0;
#pragma unroll 1
        for (int k = 0; k < N; k++) {
            const double k1 = ex.dot(row, x, c0);
            if (k == 0) first = k1;
            if (k1 > mx) { mx = k1; imx = k; }
            if (k1 < mn) { mn = k1; imn = k; }
            blown = blown || !(fabs(k1) <= TR_BLOWUP);
            if (k == next) {
                if (store) { a.y[at] = k1; at += total; }
                next += a.stride;
            }
            x = rk4_finish<P>(ex, row, c0, state, x, k1, dt, hdt, dt6);
        }
        last = ex.dot(row, x, c0);
        if (last > mx) { mx = last; imx = N; }
        if (last < mn) { mn = last; imn = N; }
        blown = blown || !(fabs(last) <= TR_BLOWUP);
        if (store) a.y[(int64_t)(a.ns - 1) * total + q] = last;
    }
    const bool diverged = g.any(outlane && blown);

    // ---- y0, yf, dir, stepsize: fixed from here on (on the output lane; the other lanes' values are never used)
    const double nan = __builtin_nan("");
    const double y0g = a.y0_in ? a.y0_in[q] : nan, yfg = a.yf_in ? a.yf_in[q] : nan;
    const double y0 = y0g != y0g ? first : y0g, yf = yfg != yfg ? last : yfg;
    const double stepsize = fabs(yf - y0);
    const bool flat = !(stepsize > 0.0) || !is_fin(stepsize);
    const bool down = !flat && yf - y0 < 0.0;   // (a flat pair is described with dir = +1)
    const double dir = down ? -1.0 : 1.0;
    const double lo_t = a.rise_lo * stepsize, hi_t = a.rise_hi * stepsize, band = a.settling_th * stepsize;

    // ---- pass 2: the same trajectory again; first crossings and the last sample outside the band
    int ilo = -1, ihi = -1, iout = -1;
    {
        double x = 0.0;
#pragma unroll 1
        for (int k = 0; k < N; k++) {
            const double k1 = ex.dot(row, x, c0);
            const double e = dir * (k1 - y0);
            if (ilo < 0 && e > lo_t) ilo = k;
            if (ihi < 0 && e > hi_t) ihi = k;
            if (fabs(k1 - yf) > band) iout = k;
            x = rk4_finish<P>(ex, row, c0, state, x, k1, dt, hdt, dt6);
        }
        const double v = ex.dot(row, x, c0);
        const double e = dir * (v - y0);
        if (ilo < 0 && e > lo_t) ilo = N;
        if (ihi < 0 && e > hi_t) ihi = N;
        if (fabs(v - yf) > band) iout = N;
    }
    if (!valid || !outlane) return;

    const double peak = down ? mn : mx;
    const int ipeak = down ? imn : imx;
    const int iset = iout < 0 ? 0 : (iout + 1 < N ? iout + 1 : N);
    double out[9];
    out[0] = y0; out[1] = yf; out[2] = stepsize; out[3] = peak; out[4] = (double)ipeak * dt;
    out[5] = dir * 100.0 * (peak - yf) / stepsize;
    out[6] = fmax(0.0, 100.0 * (down ? mx - y0 : y0 - mn) / stepsize);
    out[7] = (double)iset * dt;
    out[8] = (ilo < 0 || ihi < 0) ? nan : (double)(ihi - ilo) * dt;
    int32_t st = 0;
    if (diverged) {
        st = FB_STEPINFO_DIVERGED;
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = nan;
    } else if (flat) {
        st = FB_STEPINFO_FLAT;
#pragma unroll
        for (int k = 5; k < 9; k++) out[k] = nan;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) a.info[(int64_t)k * total + q] = out[k];
    a.status[q] = st;
}

}  // namespace fbt

// k_timeresp_map: the same call on a sampled model (fb_lss_c2d; docs/design/linearize.md, "Sampled models on the device"; numpy
// restatement: tests/c2d_prototype.py). The handle's copy holds Phi in A's place and Gamma in B's: x_{k+1} = Phi x_k + gamma, gamma =
// Gamma[:, iu], y_k = c x_k + d, from rest, samples at t_k = k Ts. Pairs, lanes, passes, arguments, outputs and status words are
// k_timeresp's; the ONE broadcast dot product of sample k is x_{k+1} on the state lanes and y_k on the output lane, so a pass takes
// N + 1 exchanges where RK4 takes 4 N + 1. (Its own namespace: fbt:: is the set of the RK4 instances.)
namespace fbz {

template <int P>
__global__ __launch_bounds__(fbt::TR_WAVE) void k_timeresp_map(fbt::TimeRespArgs a) {
    using namespace fbg;
    __shared__ __attribute__((aligned(16))) double panel[fbt::TR_WAVE];
    const fbg::Lanes<P> g;
    constexpr int NG = fbt::TR_WAVE / P;
    const int r = g.r, nx = a.nx, N = a.nsteps;
    const int64_t total = a.n * a.m;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n, j = q / a.n;
    const int iu = a.iu[j], iy = a.iy[j];
    const int64_t S = a.n * a.G, slot0 = i * a.G;

    // this lane's row: of Phi, or the output row
    const bool state = r < nx, outlane = r == nx;
    double row[P];
#pragma unroll
    for (int c = 0; c < P; c++) {
        double v = 0.0;
        if (c < nx) {
            if (state) v = a.ab[ab_index(S, slot0, c) + r];
            else if (outlane) v = a.cd[cd_index(a.n, i, a.ny, iy, c)];
        }
        row[c] = v;
    }
    const double c0 = state ? a.ab[ab_index(S, slot0, a.G + iu) + r] : outlane ? a.cd[cd_index(a.n, i, a.ny, iy, nx + iu)] : 0.0;
    const double dt = a.dt;
    const fbg::Exchange<P, 0> ex(panel);

    // ---- pass 1: endpoints, extrema at their first index, blow-up; the samples asked for
    double first = 0.0, last = 0.0, mx = -__builtin_inf(), mn = __builtin_inf();
    int imx = 0, imn = 0;
    bool blown = false;
    {
        const bool store = a.y != nullptr && valid && outlane;
        int64_t at = q;
        int next = 0;
        double x = 0.0;
#pragma unroll 1
        for (int k = 0; k < N; k++) {
            const double v = ex.dot(row, x, c0);
            if (k == 0) first = v;
            if (v > mx) { mx = v; imx = k; }
            if (v < mn) { mn = v; imn = k; }
            blown = blown || !(fabs(v) <= fbt::TR_BLOWUP);
            if (k == next) {
                if (store) { a.y[at] = v; at += total; }
                next += a.stride;
            }
            x = state ? v : 0.0;   // (a lane without a state publishes 0)
        }
        last = ex.dot(row, x, c0);
        if (last > mx) { mx = last; imx = N; }
        if (last < mn) { mn = last; imn = N; }
        blown = blown || !(fabs(last) <= fbt::TR_BLOWUP);
        if (store) a.y[(int64_t)(a.ns - 1) * total + q] = last;
    }
    const bool diverged = g.any(outlane && blown);

    // ---- y0, yf, dir, stepsize: fixed from here on (on the output lane; the other lanes' values are never used)
    const double nan = __builtin_nan("");
    const double y0g = a.y0_in ? a.y0_in[q] : nan, yfg = a.yf_in ? a.yf_in[q] : nan;
    const double y0 = y0g != y0g ? first : y0g, yf = yfg != yfg ? last : yfg;
    const double stepsize = fabs(yf - y0);
    const bool flat = !(stepsize > 0.0) || !is_fin(stepsize);
    const bool down = !flat && yf - y0 < 0.0;   // (a flat pair is described with dir = +1)
    const double dir = down ? -1.0 : 1.0;
    const double lo_t = a.rise_lo * stepsize, hi_t = a.rise_hi * stepsize, band = a.settling_th * stepsize;

    // ---- pass 2: the same trajectory again; first crossings and the last sample outside the band
    int ilo = -1, ihi = -1, iout = -1;
    {
        double x = 0.0;
#pragma unroll 1
        for (int k = 0; k < N; k++) {
            const double v = ex.dot(row, x, c0);
            const double e = dir * (v - y0);
            if (ilo < 0 && e > lo_t) ilo = k;
            if (ihi < 0 && e > hi_t) ihi = k;
            if (fabs(v - yf) > band) iout = k;
            x = state ? v : 0.0;
        }
        const double v = ex.dot(row, x, c0);
        const double e = dir * (v - y0);
        if (ilo < 0 && e > lo_t) ilo = N;
        if (ihi < 0 && e > hi_t) ihi = N;
        if (fabs(v - yf) > band) iout = N;
    }
    if (!valid || !outlane) return;

    const double peak = down ? mn : mx;
    const int ipeak = down ? imn : imx;
    const int iset = iout < 0 ? 0 : (iout + 1 < N ? iout + 1 : N);
    double out[9];
    out[0] = y0; out[1] = yf; out[2] = stepsize; out[3] = peak; out[4] = (double)ipeak * dt;
    out[5] = dir * 100.0 * (peak - yf) / stepsize;
    out[6] = fmax(0.0, 100.0 * (down ? mx - y0 : y0 - mn) / stepsize);
    out[7] = (double)iset * dt;
    out[8] = (ilo < 0 || ihi < 0) ? nan : (double)(ihi - ilo) * dt;
    int32_t st = 0;
    if (diverged) {
        st = FB_STEPINFO_DIVERGED;
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = nan;
    } else if (flat) {
        st = FB_STEPINFO_FLAT;
#pragma unroll
        for (int k = 5; k < 9; k++) out[k] = nan;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) a.info[(int64_t)k * total + q] = out[k];
    a.status[q] = st;
}

}  // namespace fbz
