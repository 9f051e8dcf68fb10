// dpid_kernels.hpp — the metrics of optimize_PID for a batch of SAMPLED linear models and PID candidates under the sampled law the stepper
// flies (include/flightbatch.h: fb_lss_dpid_metrics; host side: fb_dpid.inc; docs/design/linearize.md, "Discrete PID design on the
// device"; numpy restatement: tests/dpid_prototype.py). Reference: f_periodic! of PID, FP/control.jl:431-471, run every dt = 0.02 by
// Cessna172Xv2 and Robot2D; the metrics are FA design/pidopt.jl's (:36-70), as fbp::k_pid_metrics evaluates them on the continuous compensator.
//   plant     channel (iu, iy) of a sampled handle in deviation coordinates: Phi, gamma = Gamma[:, iu], c = C[iy, :], d = D[iy, iu]
//   point     p = (k_p, k_i, k_d, tau_f), tau_f >= 0; alpha = 1 / (tau_f + Ts); optional output bounds lo < hi (either may be infinite)
//   tick k    s_k = c x_k, r = 1 from rest, xi_-1 = eta_-1 = 0, sat_-1 = 0, k = 0 .. N
//             unbounded pair (the algebraic loop through d solved): Dc = k_p + Ts k_i + alpha k_d, g = 1 / (1 + d Dc),
//                 u_k = g (Dc (1 - s_k) + xi_k-1 - alpha eta_k-1),  e_k = 1 - s_k - d u_k,  xi_k = xi_k-1 + Ts k_i e_k
//             pair with a finite bound (d = 0): e_k = 1 - s_k, halted_k = e_k sat_k-1 > 0, xi_k = xi_k-1 (halted) or xi_k-1 + Ts k_i e_k,
//                 free_k = k_p e_k + xi_k + alpha (k_d e_k - eta_k-1), u_k = clamp(free_k, lo, hi), sat_k = (free_k >= hi) - (free_k <= lo)
//             both: eta_k = alpha tau_f eta_k-1 + Ts alpha k_d e_k,  y_k = s_k + d u_k,  x_k+1 = Phi x_k + gamma u_k
//   metrics   fbp::k_pid_metrics' (Ms, ie, ef, iu, up) on the samples y_k, u_k; Ms = min(1e3, max_j 1 / |1 + P(z_j) C(z_j)|) with
//             C(z) = k_p + k_i Ts z / (z - 1) + k_d alpha (z - 1) / (z - alpha tau_f), the LINEAR law's: the bounds play no part in it.
//             The grid arrives as cos and sin of w_j Ts (the host's): no trigonometric function is evaluated here.
// k_dpid_metrics: one (system, candidate) pair per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx + 1). Lanes 0 .. nx - 1
// own the rows of Phi and their gamma_r, lane nx owns c: ONE broadcast dot product of x_k per tick (Exchange<P, 0>) is Phi_r x_k on the state
// lanes and s_k on lane nx, one cross-lane read hands s_k to the group, and every lane carries xi, eta and sat redundantly, so the law is
// uniform in the group and x_k+1,r = fma(gamma_r, u_k, Phi_r x_k) needs no second exchange (fbp::k_pid_metrics takes four per sample).
// The bounded law is a branch that is uniform within a group: a pair's arithmetic does not depend on what its wave neighbours are.
// Lanes past the batch's end work on the last pair again and store nothing, so a wave never diverges on the batch size.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbu {

using namespace fbg;

constexpr double DPID_MS_MAX = 1e3;      // pidopt.jl:43
constexpr double DPID_BLOWUP = 1e12;     // |y| or |u| beyond this: FB_DPID_DIVERGED

struct DPidArgs {
    const double* ab; const double* cd;   // the handle's copies (fbg::ab_index, lss_group.hpp), G its group size: Phi | Gamma, C | D
    const double* cs; const double* sn;   // [nw]: cos(w_j Ts), sin(w_j Ts)
    const double* pre; const double* pim; // P(z_j) on the grid, [nw x n] (fbw::k_lss_dfreqresp)
    const double* pid;                    // [4 x m x n]: k_p, k_i, k_d, tau_f
    const double* bounds;                 // [2 x m x n]: lo, hi; or null (-Inf, +Inf)
    double* metrics;                      // [5 x m x n] (Ms, ie, ef, iu, up), may be null
    double* cost;                         // [m x n]
    int32_t* counts;                      // [2 x m x n]: ticks with sat != 0, ticks with the integrator halted; may be null
    int32_t* status;                      // [m x n]
    int64_t n;
    int nx, nu, ny, G, iu, iy, nw, m, nticks;   // nticks = N: the samples are k = 0 .. N
    double Ts;
    double wt[5], wsum;
};

template <int P>
__global__ __launch_bounds__(WAVE) void k_dpid_metrics(DPidArgs a) {
    __shared__ __attribute__((aligned(16))) double panel[WAVE];
    const Lanes<P> g;
    constexpr int NG = WAVE / P;
    const int r = g.r, nx = a.nx;
    const int64_t total = a.n * a.m;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const double kp = a.pid[q], ki = a.pid[total + q], kd = a.pid[2 * total + q], tf = a.pid[3 * total + q];
    const double lo = a.bounds ? a.bounds[q] : -inf, hi = a.bounds ? a.bounds[total + q] : inf;
    const double d = a.cd[cd_index(a.n, i, a.ny, a.iy, nx + a.iu)];
    const double Ts = a.Ts, al = 1.0 / (tf + Ts), alkd = al * kd, altf = al * tf, tski = Ts * ki, tsalkd = Ts * alkd;
    const double Dc = kp + tski + alkd, den = 1.0 + d * Dc, gg = 1.0 / den;
    const bool bounded = is_fin(lo) || is_fin(hi);
    const bool direct = bounded && d != 0.0;
    const bool singular_loop = !bounded && (!(den != 0.0) || !is_fin(gg));

    // this lane's row: Phi_r and gamma_r on the state lanes, c on lane nx, zeros past it
    const bool plant = r < nx;
    const double gam = plant ? a.ab[ab_index(S, slot0, a.G + a.iu) + r] : 0.0;
    double row[P];
#pragma unroll
    for (int c = 0; c < P; c++) {
        double v = 0.0;
        if (c < nx) {
            if (plant) v = a.ab[ab_index(S, slot0, c) + r];
            else if (r == nx) v = a.cd[cd_index(a.n, i, a.ny, a.iy, c)];
        }
        row[c] = v;
    }

    // ---- the step response: ticks k = 0 .. N of the law around the exact map
    const Exchange<P, 0> ex(panel);
    const int N = a.nticks;
    double x = 0.0, xi = 0.0, eta = 0.0, sat = 0.0;
    double sy = 0.0, su = 0.0, peak = 0.0, last = 0.0;
    int nsat = 0, nhalt = 0;
    bool blown = false;
#pragma unroll 1
    for (int k = 0; k <= N; k++) {
        const double v = ex.dot(row, x, 0.0);
        const double s = __shfl(v, nx, P);
        const double one_s = 1.0 - s;
        double u, e;
        if (bounded) {
            e = one_s;
            const bool halted = e * sat > 0.0;
            xi = halted ? xi : fma(tski, e, xi);
            const double fr = fma(kp, e, xi) + al * fma(kd, e, -eta);
            u = fr == fr ? fmin(fmax(fr, lo), hi) : fr;
            sat = (fr >= hi ? 1.0 : 0.0) - (fr <= lo ? 1.0 : 0.0);
            nsat += sat != 0.0;
            nhalt += halted;
        } else {
            u = gg * (fma(Dc, one_s, xi) - al * eta);
            e = fma(-d, u, one_s);
            xi = fma(tski, e, xi);
        }
        eta = fma(altf, eta, tsalkd * e);
        const double y = fma(d, u, s);
        x = plant ? fma(gam, u, v) : 0.0;
        const double fy = fabs(y - 1.0), fu = fabs(u - 1.0);
        const double wk = (k == 0 || k == N) ? 0.5 : 1.0;
        sy = fma(wk, fy, sy);
        su = fma(wk, fu, su);
        peak = fmax(peak, fu);
        last = fy;
        blown = blown || !(fabs(y) <= DPID_BLOWUP) || !(fabs(u) <= DPID_BLOWUP);
    }
    const double ie = sy / (double)N, iu = su / (double)N;   // trapz / t_N = Ts (f_0 / 2 + f_1 + .. + f_N / 2) / (N Ts)

    // ---- Ms on the grid: the group's lanes share the frequencies
    double smax = 0.0;
    bool badp = false;
    for (int j = r; j < a.nw; j += P) {
        const double cz = a.cs[j], sz = a.sn[j], pr = a.pre[(int64_t)j * a.n + i], pi = a.pim[(int64_t)j * a.n + i];
        badp = badp || !is_fin(pr) || !is_fin(pi);
        // z / (z - 1) = 1 / (1 - 1 / z) = ((1 - cos) - j sin) / |.|^2;  (z - 1) / (z - q), q = alpha tau_f < 1
        const double ar = 1.0 - cz, im2 = fma(ar, ar, sz * sz);
        const double qr = cz - altf, qm2 = fma(qr, qr, sz * sz);
        const double dr = (fma(-ar, qr, sz * sz)) / qm2, di = (sz * qr + ar * sz) / qm2;
        const double cr = kp + tski * (ar / im2) + alkd * dr, ci = alkd * di - tski * (sz / im2);
        const double lr = 1.0 + (pr * cr - pi * ci), li = pr * ci + pi * cr;
        smax = fmax(smax, 1.0 / sqrt(fma(lr, lr, li * li)));
    }
    smax = g.gmax(smax);
    const bool singular = singular_loop || g.any(badp);
    if (!valid || r != 0) return;
    double mt[5] = {fmin(smax, DPID_MS_MAX), ie, last, iu, peak};
    double cost = 0.0;
    int32_t st = 0;
    if (direct || singular) {
        st = direct ? FB_DPID_DIRECT : FB_DPID_SINGULAR;
#pragma unroll
        for (int k = 0; k < 5; k++) mt[k] = nan;
        cost = inf;
        nsat = nhalt = 0;
    } else if (blown) {
        st = FB_DPID_DIVERGED;
#pragma unroll
        for (int k = 1; k < 5; k++) mt[k] = inf;
        cost = inf;
    } else {
#pragma unroll
        for (int k = 0; k < 5; k++) cost = fma(a.wt[k], mt[k], cost);
        cost = cost / a.wsum;
    }
    if (a.metrics) {
#pragma unroll
        for (int k = 0; k < 5; k++) a.metrics[(int64_t)k * total + q] = mt[k];
    }
    if (a.counts) { a.counts[q] = nsat; a.counts[total + q] = nhalt; }
    a.cost[q] = cost;
    a.status[q] = st;
}

}  // namespace fbu
