// pid_kernels.hpp — the metrics of optimize_PID for a batch of linear models and PID candidates on the device (include/flightbatch.h:
// fb_lss_freqresp, fb_pid_metrics; host side: fb_pid.inc; docs/design/linearize.md, "PID loop design on the device"; numpy restatement:
// tests/pid_prototype.py). Reference: FA design/pidopt.jl — build_PID :31-34, Metrics :36-64, cost :66-70; called at every node of the gain
// schedule by design/c172/c172x_design.jl:236 (q2e), and for v2t, c2theta, p2phi, chi2phi.
//   plant     channel (iu, iy) of a Model(lss) system in deviation coordinates: A, b = B[:, iu], c = C[iy, :], d = D[iy, iu]
//   PID       C(s) = k_p + k_i / s + k_d s / (tau_f s + 1):  xi' = e, eta' = (e - eta) / tau_f, u = k_p e + k_i xi + (k_d / tau_f)(e - eta),
//             e = r - y, y = c x + d u;  with Dc = k_p + k_d / tau_f and g = 1 / (1 + d Dc): u = g (Dc (r - c x) + k_i xi - (k_d / tau_f) eta)
//   metrics   step response r = 1 from rest, samples t_k = k dt, k = 0 .. N (classical RK4):  ie = trapz|y - 1| / t_N, ef = |y_N - 1|,
//             iu = trapz|u - 1| / t_N, up = max_k |u_k - 1| (the reference's expression, its "- 1" on the control signal included, :54-60);
//             Ms = min(1e3, max_j 1 / |1 + P(j w_j) C(j w_j)|) over the caller's grid, P(jw) = c inv(jw I - A) b + d;  cost = sum w m / sum w
// Differences from the reference: ControlSystems.step picks its own sample time and discretises exactly, here dt is the caller's and the
// integrator is RK4 (the exact map exists since fb_lss_c2d, c2d_kernels.hpp; these metrics on it are the follow-up); hinfnorm2 finds the exact peak and is infinite (-> 1e3) for an unstable loop, here Ms is the grid's peak and an
// unstable loop shows as FB_PID_DIVERGED; NLopt's optimisers are not restated (the search is host-side, flightbatch/pidopt.py).
//
// k_lss_freqresp: one (system, frequency) pair per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx); lane r owns the complex
// row r of [jw I - A | b]. Gauss-Jordan with the family's pivot rule (fbg::Lanes::pivot, lss_group.hpp) on |z|^2; the scaled pivot row goes through the group's LDS panel and is read back as 16-byte
// broadcasts. Every step has a compile-time index: the rows are register arrays.
// k_pid_metrics: one (system, candidate) pair per group of P lanes (P >= nx + 4). Lanes 0 .. nx + 1 own the rows of the closed loop (the plant
// rows with the rank-one feedback folded in, then xi, then eta), lanes nx + 2 and nx + 3 the output rows of y and u: the broadcast dot
// product that is the first stage of a step is, on those two lanes, the sample y_k, u_k. Stage values travel as in k_lss_rk4 (Exchange<G, 0>).
// Lanes past the batch's end work on the last pair again and store nothing, so a wave never diverges on the batch size.
#pragma once
#include "lss_group.hpp"
#include "lqr_kernels.hpp"   // fbq::Group: k_lss_freqresp uses its panels

namespace fbp {

using fbq::Group;
using namespace fbg;

constexpr int PID_WAVE = fbg::WAVE;
constexpr double PID_MS_MAX = 1e3;      // pidopt.jl:43
constexpr double PID_BLOWUP = 1e12;     // |y| or |u| beyond this: FB_PID_DIVERGED

struct FreqArgs {
    const double* ab; const double* cd;   // the handle's copies (fbg::ab_index, lss_group.hpp), G its group size
    const double* w;                      // [nw]
    double *re, *im;                      // [nw x n], system index fastest; NaN where a pivot was zero or not finite
    int64_t n;
    int nx, nu, ny, G, iu, iy, nw;
};

struct PidArgs {
    const double* ab; const double* cd;
    const double* w; const double* pre; const double* pim;   // the grid and P(jw) on it, [nw x n]
    const double* pid;                    // [4 x m x n]: k_p, k_i, k_d, tau_f
    double* metrics;                      // [5 x m x n] (Ms, ie, ef, iu, up), may be null
    double* cost;                         // [m x n]
    int32_t* status;                      // [m x n]
    int64_t n;
    int nx, nu, ny, G, iu, iy, nw, m, nsteps;
    double dt;
    double wt[5], wsum;
};

template <int P>
__global__ __launch_bounds__(PID_WAVE) void k_lss_freqresp(FreqArgs a) {
    using Grp = Group<P>;
    constexpr int NG = PID_WAVE / P;
    __shared__ __attribute__((aligned(16))) double lds_d[NG * (Grp::PANEL + 2 * Grp::SIDE)];
    __shared__ int lds_i[PID_WAVE];
    const Grp g(lds_d, lds_i);
    const int r = g.r, nx = a.nx;
    const int64_t total = a.n * a.nw;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n, iw = q / a.n;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const bool live = r < nx;
    const double om = a.w[iw];

    double zr[P], zi[P];
#pragma unroll
    for (int c = 0; c < P; c++) {
        zr[c] = (live && c < nx) ? -a.ab[ab_index(S, slot0, c) + r] : 0.0;
        zi[c] = c == r ? om : 0.0;
    }
    double br = live ? a.ab[ab_index(S, slot0, a.G + a.iu) + r] : 0.0, bi = 0.0;

    bool used = !live, ok = true;
    int myk = r;
    double2* pan = reinterpret_cast<double2*>(g.pan);   // P + 1 complex numbers: the scaled pivot row, its right-hand side last
#pragma unroll
    for (int k = 0; k < P; k++) {
        if (k < nx) {
            const Pivot pv = g.pivot(used, used ? -1.0 : fma(zr[k], zr[k], zi[k] * zi[k]), k);
            ok = ok && pv.found;
            panel_sync();
            if (r == pv.p) {
                const double ipr = zr[k] / pv.m, ipi = -zi[k] / pv.m;   // 1 / z = conj(z) / |z|^2
#pragma unroll
                for (int j = k + 1; j < P; j++) {
                    const double sr = zr[j] * ipr - zi[j] * ipi, si = zr[j] * ipi + zi[j] * ipr;
                    zr[j] = sr; zi[j] = si;
                    pan[j] = make_double2(sr, si);
                }
                const double sr = br * ipr - bi * ipi, si = br * ipi + bi * ipr;
                br = sr; bi = si;
                pan[P] = make_double2(sr, si);
                used = true; myk = k;
            }
            panel_sync();
            if (r != pv.p) {
                const double fr = zr[k], fi = zi[k];
#pragma unroll
                for (int j = k + 1; j < P; j++) {
                    const double2 s = pan[j];
                    zr[j] = fma(-fr, s.x, fma(fi, s.y, zr[j]));
                    zi[j] = fma(-fr, s.y, fma(-fi, s.x, zi[j]));
                }
                const double2 s = pan[P];
                br = fma(-fr, s.x, fma(fi, s.y, br));
                bi = fma(-fr, s.y, fma(-fi, s.x, bi));
            }
        }
    }
    // the lane that was the pivot of step k holds x_k: P(jw) = d + sum_k c_k x_k, k ascending
    double2* xs = reinterpret_cast<double2*>(g.ya);
    panel_sync();
    if (live) xs[myk] = make_double2(br, bi);
    panel_sync();
    double pr = a.cd[cd_index(a.n, i, a.ny, a.iy, nx + a.iu)], pi = 0.0;
    for (int k = 0; k < nx; k++) {
        const double ck = a.cd[cd_index(a.n, i, a.ny, a.iy, k)];
        const double2 x = xs[k];
        pr = fma(ck, x.x, pr);
        pi = fma(ck, x.y, pi);
    }
    ok = ok && is_fin(pr) && is_fin(pi);
    if (!valid || r != 0) return;
    const double nan = __builtin_nan("");
    a.re[q] = ok ? pr : nan;
    a.im[q] = ok ? pi : nan;
}

template <int P>
__global__ __launch_bounds__(PID_WAVE) void k_pid_metrics(PidArgs a) {
    __shared__ __attribute__((aligned(16))) double panel[PID_WAVE];
    const fbg::Lanes<P> g;
    constexpr int NG = PID_WAVE / P;
    const int r = g.r, nx = a.nx;
    const int64_t total = a.n * a.m;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const double kp = a.pid[q], ki = a.pid[total + q], kd = a.pid[2 * total + q], tf = a.pid[3 * total + q];
    const double d = a.cd[cd_index(a.n, i, a.ny, a.iy, nx + a.iu)];
    const double kdt = kd / tf, Dc = kp + kdt, den = 1.0 + d * Dc, gg = 1.0 / den;
    const bool singular_loop = !(den != 0.0) || !is_fin(gg);
    const double uc = gg * Dc, yc = d * uc;   // u = uc + urow . z, y = yc + yrow . z with z = (x, xi, eta)

    // this lane's row of the closed loop, or of the outputs
    const bool plant = r < nx, state = r < nx + 2;
    const double br = plant ? a.ab[ab_index(S, slot0, a.G + a.iu) + r] : 0.0;
    double row[P];
#pragma unroll
    for (int c = 0; c < P; c++) {
        const double cc = c < nx ? a.cd[cd_index(a.n, i, a.ny, a.iy, c)] : 0.0;
        const double ur = gg * (c < nx ? -Dc * cc : c == nx ? ki : c == nx + 1 ? -kdt : 0.0);
        const double yr = cc + d * ur;
        double v = 0.0;
        if (plant) v = (c < nx ? a.ab[ab_index(S, slot0, c) + r] : 0.0) + br * ur;
        else if (r == nx) v = -yr;
        else if (r == nx + 1) v = (-yr - (c == nx + 1 ? 1.0 : 0.0)) / tf;
        else if (r == nx + 2) v = yr;
        else if (r == nx + 3) v = ur;
        row[c] = v;
    }
    const double c0 = plant ? br * uc : r == nx ? 1.0 - yc : r == nx + 1 ? (1.0 - yc) / tf : r == nx + 2 ? yc : r == nx + 3 ? uc : 0.0;

    // ---- the step response: N steps of RK4; the first stage of step k is, on the output lanes, sample k
    const double dt = a.dt, hdt = a.dt / 2, dt6 = a.dt / 6;
    const fbg::Exchange<P, 0> ex(panel);
    double x = 0.0, sum = 0.0, peak = 0.0, last = 0.0;
    bool blown = false;
#pragma unroll 1
    for (int k = 0; k < a.nsteps; k++) {
        const double k1 = ex.dot(row, x, c0);
        const double f = fabs(k1 - 1.0);
        sum += k == 0 ? 0.5 * f : f;
        peak = fmax(peak, f);
        blown = blown || !(fabs(k1) <= PID_BLOWUP);
        x = fbg::rk4_finish<P>(ex, row, c0, state, x, k1, dt, hdt, dt6);
    }
    {
        const double v = ex.dot(row, x, c0);
        last = fabs(v - 1.0);
        sum += 0.5 * last;
        peak = fmax(peak, last);
        blown = blown || !(fabs(v) <= PID_BLOWUP);
    }
    const bool outlane = r == nx + 2 || r == nx + 3;
    const bool diverged = g.any(outlane && blown);
    const double mean = sum / (double)a.nsteps;   // trapz / t_N = dt (f_0 / 2 + f_1 + .. + f_N / 2) / (N dt)
    const int ly = g.base + nx + 2, lu = ly + 1;  // (a group never straddles the wave)
    const double ie = __shfl(mean, ly), ef = __shfl(last, ly), iu = __shfl(mean, lu), up = __shfl(peak, lu);

    // ---- Ms on the grid: the group's lanes share the frequencies
    double smax = 0.0;
    bool badp = false;
    for (int j = r; j < a.nw; j += P) {
        const double om = a.w[j], pr = a.pre[(int64_t)j * a.n + i], pi = a.pim[(int64_t)j * a.n + i];
        badp = badp || !is_fin(pr) || !is_fin(pi);
        const double dd = fma(om * tf, om * tf, 1.0);
        const double cr = kp + kd * om * om * tf / dd, ci = kd * om / dd - ki / om;
        const double lr = 1.0 + (pr * cr - pi * ci), li = pr * ci + pi * cr;
        smax = fmax(smax, 1.0 / sqrt(fma(lr, lr, li * li)));
    }
    smax = g.gmax(smax);
    const bool singular = singular_loop || g.any(badp);
    if (!valid || r != 0) return;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    double mt[5] = {fmin(smax, PID_MS_MAX), ie, ef, iu, up};
    double cost = 0.0;
    int32_t st = 0;
    if (singular) {
        st = FB_PID_SINGULAR;
#pragma unroll
        for (int k = 0; k < 5; k++) mt[k] = nan;
        cost = inf;
    } else if (diverged) {
        st = FB_PID_DIVERGED;
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
    a.cost[q] = cost;
    a.status[q] = st;
}

}  // namespace fbp
