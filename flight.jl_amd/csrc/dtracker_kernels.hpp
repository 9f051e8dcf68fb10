// dtracker_kernels.hpp — the sampled LQR tracker law the stepper flies, on a batch of SAMPLED linear models and gain candidates
// (include/flightbatch.h: fb_lss_dtracker_metrics; host side: fb_dtracker.inc; docs/design/linearize.md, "Discrete LQR trackers on the
// device"; numpy restatement: tests/dtracker_prototype.py). Reference: f_periodic! of LQR, FP/control.jl:708-743, run every dt = 0.02 by
// Cessna172Xv2 (te2te, tv2te, vh2te, ar2ar, phibeta2ar) and Robot2D, with sat_ext = 0 and x_trim, u_trim, z_trim at the origin.
//   plant     a sampled handle in deviation coordinates: Phi, Gamma, C_z = C[iz, :], D_z = D[iz, :]
//   pair      K_fbk [nu x nx], K_fwd [nu x nz], K_int [nu x nz]; optional output bounds lo < hi per input (either may be infinite)
//   tick k    z_k = C_z x_k + D_z u_k-1,  e_k = zref - z_k,  v_k = K_int e_k,  halted_kj = v_kj sat_k-1,j > 0,
//             iota_kj = iota_k-1,j (halted) or iota_k-1,j + Ts v_kj,  free_k = iota_k + K_fwd zref - K_fbk x_k,
//             sat_k = (free_k >= hi) - (free_k <= lo),  u_k = clamp(free_k, lo, hi),  x_k+1 = Phi x_k + Gamma u_k;  k = 0 .. N from rest
//   metrics   per command variable: the trapezoid mean of |e|, the last |e|, max |z|; per input: the trapezoid mean of |u|, max |u|, the ticks
//             with sat != 0 and the ticks with the integrator halted
// k_dtracker: one (system, candidate) pair per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx + nu + nz). Lanes
// 0 .. nx - 1 own the rows of Phi with their row of Gamma, the next nu lanes the rows of K_fbk with their row of K_int (and carry iota_j and
// sat_j), the next nz lanes the rows of C_z with their row of D_z: ONE broadcast dot product of x_k per tick (Exchange<P, 0>) is Phi_r x_k,
// K_fbk,j x_k and C_z,c x_k at once; the nz errors and the nu outputs then travel by cross-lane reads. Every sum is an explicit fma chain in
// ascending index, so a pair's bits do not depend on its wave, its group or its neighbours. There is one law: without bounds lo = -Inf and
// hi = +Inf, under which sat stays 0, nothing halts and the clamp returns its argument. Lanes past the batch's end work on the last pair
// again and store nothing, so a wave never diverges on the batch size.
#pragma once
#include "lss_group.hpp"
#include "surgery_kernels.hpp"
#include "../../include/flightbatch.h"

namespace fbj {

using namespace fbg;

constexpr int DT_W = 8;                  // the inputs and the command variables of a pair: at most 8 each
constexpr double DTRACK_BLOWUP = 1e12;   // |z| or |u| beyond this: FB_DTRACK_DIVERGED

struct DTrackArgs {
    const double* ab; const double* cd;   // the handle's copies (fbg::ab_index, lss_group.hpp), G its group size: Phi | Gamma, C | D
    const int32_t* iz;                    // [nz] rows of the outputs
    const double* kfbk;                   // [nu x nx x m x n]: element (r, c) of pair q at [(r + nu c) m n + q]
    const double* kfwd; const double* kint;   // [nu x nz x m x n], the same rule
    const double* bounds;                 // [2 x nu x m x n]: lo, hi; or null (-Inf, +Inf)
    const double* zref;                   // [nz]
    double *zmet, *umet;                  // [3 x nz x m x n] (ie, ef, zp), [2 x nu x m x n] (iu, up); each may be null
    int32_t* counts;                      // [2 x nu x m x n]: ticks with sat != 0, ticks with the integrator halted; may be null
    double *zs, *us;                      // [ns x nz x m x n], [ns x nu x m x n]: sample s stride at row s, sample N at row ns - 1; each may be null
    int32_t* status;                      // [m x n]
    int64_t n;
    int nx, nu, ny, G, nz, m, nticks, stride;   // nticks = N: the samples are k = 0 .. N
    double Ts;
};

template <int P>
__global__ __launch_bounds__(WAVE) void k_dtracker(DTrackArgs a) {
    __shared__ __attribute__((aligned(16))) double panel[WAVE];
    const Lanes<P> g;
    constexpr int NG = WAVE / P;
    const int r = g.r, nx = a.nx, nu = a.nu, nz = a.nz;
    const int64_t total = a.n * a.m;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const bool plant = r < nx, ctl = r >= nx && r < nx + nu, out = r >= nx + nu && r < nx + nu + nz;
    const int jr = ctl ? r - nx : 0, cr = out ? r - nx - nu : 0;
    const int zrow = out ? a.iz[cr] : 0;

    // this lane's row: Phi_r | Gamma_r, K_fbk,j | K_int,j or C_z,c | D_z,c; zeros past it
    bool fin = true;
    double row[P], aux[DT_W];
#pragma unroll
    for (int c = 0; c < P; c++) {
        double v = 0.0;
        if (c < nx) {
            if (plant) v = a.ab[ab_index(S, slot0, c) + r];
            else if (ctl) v = a.kfbk[(jr + (int64_t)nu * c) * total + q];
            else if (out) v = a.cd[cd_index(a.n, i, a.ny, zrow, c)];
        }
        fin = fin && is_fin(v);
        row[c] = v;
    }
#pragma unroll
    for (int c = 0; c < DT_W; c++) {
        double v = 0.0;
        if (plant && c < nu) v = a.ab[ab_index(S, slot0, a.G + c) + r];
        else if (ctl && c < nz) v = a.kint[(jr + (int64_t)nu * c) * total + q];
        else if (out && c < nu) v = a.cd[cd_index(a.n, i, a.ny, zrow, nx + c)];
        fin = fin && is_fin(v);
        aux[c] = v;
    }
    // the controller lane's feed-forward K_fwd,j zref and bounds; the output lane's zref_c
    double ff = 0.0, lo = -inf, hi = inf;
    if (ctl) {
        for (int c = 0; c < nz; c++) {
            const double kf = a.kfwd[(jr + (int64_t)nu * c) * total + q];
            fin = fin && is_fin(kf);
            ff = fma(kf, a.zref[c], ff);
        }
        if (a.bounds) { lo = a.bounds[(int64_t)jr * total + q]; hi = a.bounds[((int64_t)nu + jr) * total + q]; }
    }
    const double zr = out ? a.zref[cr] : 0.0;
    const bool bad = g.any(!fin);

    // ---- ticks k = 0 .. N of the law around the exact map
    const Exchange<P, 0> ex(panel);
    const int N = a.nticks;
    const double Ts = a.Ts;
    double x = 0.0, iota = 0.0, sat = 0.0;
    double up[DT_W];                                // u_k-1 of the pair, on every lane
#pragma unroll
    for (int c = 0; c < DT_W; c++) up[c] = 0.0;
    double sm = 0.0, peak = 0.0, last = 0.0;        // of |e_c| and |z_c| on an output lane, of |u_j| on a controller lane
    int nsat = 0, nhalt = 0, next = 0;
    int64_t srow = 0;
    bool blown = false;
#pragma unroll 1
    for (int k = 0; k <= N; k++) {
        const double v = ex.dot(row, x, 0.0);
        // z_c = C_z,c x + D_z,c u_k-1 and e_c on the output lanes; elsewhere a finite number nobody reads
        double z = v;
#pragma unroll
        for (int c = 0; c < DT_W; c++) z = fma(aux[c], up[c], z);
        const double e = zr - z;
        // v_j = K_int,j e and the law on the controller lanes
        double vi = 0.0;
#pragma unroll
        for (int c = 0; c < DT_W; c++) {
            const double ec = __shfl(e, nx + nu + c, P);
            vi = fma(aux[c], c < nz ? ec : 0.0, vi);
        }
        const bool halted = vi * sat > 0.0;
        iota = halted ? iota : fma(Ts, vi, iota);
        const double fr = (iota + ff) - v;
        const double u = fr == fr ? fmin(fmax(fr, lo), hi) : fr;
        sat = (fr >= hi ? 1.0 : 0.0) - (fr <= lo ? 1.0 : 0.0);
        // u_k to every lane, x_k+1,r = Phi_r x_k + Gamma_r u_k on the plant lanes
        double xn = v;
#pragma unroll
        for (int c = 0; c < DT_W; c++) {
            const double uc = __shfl(u, nx + c, P);
            up[c] = c < nu ? uc : 0.0;
            xn = fma(aux[c], up[c], xn);
        }
        x = plant ? xn : 0.0;
        // what the lanes keep
        const double wk = (k == 0 || k == N) ? 0.5 : 1.0;
        const double f = ctl ? fabs(u) : fabs(e), pk = ctl ? fabs(u) : fabs(z);
        sm = fma(wk, f, sm);
        peak = fmax(peak, pk);
        last = f;
        nsat += ctl && sat != 0.0;
        nhalt += ctl && halted;
        blown = blown || ((ctl || out) && !(pk <= DTRACK_BLOWUP));
        if (k == next || k == N) {
            if (valid && out && a.zs) a.zs[(srow * nz + cr) * total + q] = z;
            if (valid && ctl && a.us) a.us[(srow * nu + jr) * total + q] = u;
            srow++;
            next += a.stride;
        }
    }
    const bool div = g.any(blown);
    if (!valid) return;
    const int32_t st = bad ? FB_DTRACK_NOT_FINITE : div ? FB_DTRACK_DIVERGED : 0;
    double mean = sm / (double)N;                   // trapz / t_N = Ts (f_0 / 2 + f_1 + .. + f_N / 2) / (N Ts)
    if (st) { mean = last = peak = bad ? nan : inf; nsat = nhalt = 0; }
    if (out && a.zmet) {
        a.zmet[(int64_t)cr * total + q] = mean;
        a.zmet[((int64_t)nz + cr) * total + q] = last;
        a.zmet[(2 * (int64_t)nz + cr) * total + q] = peak;
    }
    if (ctl) {
        if (a.umet) { a.umet[(int64_t)jr * total + q] = mean; a.umet[((int64_t)nu + jr) * total + q] = peak; }
        if (a.counts) { a.counts[(int64_t)jr * total + q] = nsat; a.counts[((int64_t)nu + jr) * total + q] = nhalt; }
    }
    if (r == 0) a.status[q] = st;
}

// fb_lss_dsteady: fbm::k_steady's body on a sampled model (surgery_kernels.hpp)
template <int P>
__global__ __launch_bounds__(WAVE) void k_dsteady(fbm::SteadyArgs a) { fbm::steady_body<P, true>(a); }

}  // namespace fbj
