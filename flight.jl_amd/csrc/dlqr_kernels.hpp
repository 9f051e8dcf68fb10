// dlqr_kernels.hpp — the discrete LQR of a batch of sampled linear models on the device (include/flightbatch.h: fb_lss_dlqr; host side:
// fb_dlqr.inc; docs/design/linearize.md, "Discrete LQR on the device"; numpy restatement, operation for operation: tests/dlqr_prototype.py).
// Reference: ControlSystems' lqr(Discrete, Phi, Gamma, Q, R), the sampled-data counterpart of the design scripts' lqr(P, Q, R); the
// controllers of FP/control.jl run in f_periodic! at dt = 0.02. The algorithm is ours.
//   the equation   X = Phi' X Phi - Phi' X Gam inv(R + Gam' X Gam) Gam' X Phi + Q,   K = inv(R + Gam' X Gam) Gam' X Phi
//   doubling       A = Phi, G = Gam inv(R) Gam', H = Q;   W = I + G H,  [V | U] = inv(W) [A | G]  (one fbg::gj_solve, NE = P, NR = 2 P)
//                  H <- H + A' (H V),  G <- G + (A U) A',  A <- A V
//                  until max|dH| <= DLQR_TOL max|H| and max|A| <= DLQR_A_TOL, at most FB_DLQR_MAX_ITERS times. A_k is the closed loop over
//                  2^k samples: the second condition is the statement that the loop is stable (an unobservable mode on the unit circle
//                  leaves H converged and A where it is). Nothing is inverted but W: Phi may be singular.
//   the gain       X = (H + H') / 2;  Phic = inv(I + G0 X) Phi is the closed loop, by the same solve;  K = inv(R) (Gam' (X Phic))
//   the residual   max|Phi' (X (Phi - Gam K)) - X + Q| / max(max|Q|, max|X|)
//
// k_lss_dlqr: one system per group of P lanes of one wave (P = 8 or 16, the smallest >= nx; 64 / P systems per wave, one wave per
// workgroup); lane r owns row r of A, G and H. A product X Y keeps X's row in registers; Y's rows are published in one of the group's LDS
// panels and read back as 16-byte broadcasts, every sum an explicit fma with the columns ascending over c < nx, so a result is a function
// of the system's own values only. A' is published column by column (lane j writes column j of the panel `tp`: consecutive lanes,
// consecutive addresses); (A U) A' then reads its rows as broadcasts and A' (H V) has lane r read row r of it, eight bytes at a time: the
// row pitch P + 2 keeps those reads on different banks and the rows on 16-byte boundaries. Lanes r >= nx hold rows of zeros that nothing
// reads, the columns c >= nx of the rows r < nx stay exact zeros. The groups of a wave double a different number of times: the loop runs
// while the ballot of the groups still running is non-zero, a finished group keeps its values through selects. The panels belong to one
// wave: fences and wave_barrier, no workgroup barrier. Lanes past the batch's end design the last system again and store nothing.
// The closed model (Phi - Gam K in A's place, C - D K in C's) goes to a staging block in fb_linearize's layout when one is given;
// fbl::k_lss_gather makes the new handle's copy from it.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbk {

using namespace fbg;

constexpr int DLQR_WAVE = fbg::WAVE;
constexpr int DLQR_NU_MAX = 8;             // the inputs of a model: fbl::LSS_NU_MAX
constexpr double DLQR_TOL = 1e-13;
constexpr double DLQR_A_TOL = 0x1p-20;

struct DlqrArgs {
    const double* ab; const double* xs; const double* u0; const double* y0; const double* cd;   // the source handle's copies (fbg::ab_index)
    const double* q;        // Q, nx x nx column-major (symmetric)
    double *K, *X, *resid;  // outputs in fb_linearize's layout, any may be null
    int32_t *iters, *status;
    int64_t n;
    int nx, nu, ny, G;
    double qmax;            // max|Q|
    double rinv[DLQR_NU_MAX * DLQR_NU_MAX];   // inv(R), element (a, b) at [a nu + b] (symmetric)
    double *xdot0, *x0, *u0_out, *y0_out;     // the closed model's staging, fb_linearize's layout (AB null: no closed model is made)
    double* AB; double* CD;
};

// the LDS of one group, in doubles: two P x (P + 2) panels, the solution rows P x 2 P, the pivot row 3 P
template <int P> struct Panels {
    static constexpr int LD = P + 2, SLD = 2 * P, GRP = 2 * P * LD + P * SLD + 3 * P;
};

// this lane's row into row r of the panel w, once the reads of what it held are done; readable when this returns
template <int N, int LD>
__device__ __forceinline__ void rows_put(double* w, int r, const double (&row)[N]) {
    panel_sync();
#pragma unroll
    for (int c = 0; c < N; c++) w[r * LD + c] = row[c];
    panel_sync();
}
// this lane's row into column r of the panel: the panel then holds the transposed matrix
template <int P, int LD>
__device__ __forceinline__ void cols_put(double* w, int r, const double (&row)[P]) {
    panel_sync();
#pragma unroll
    for (int c = 0; c < P; c++) w[c * LD + r] = row[c];
    panel_sync();
}
// acc_j += sum_{c < nx} x_c W_cj, c ascending: W's rows at pitch LD, read as 16-byte broadcasts
template <int P, int LD>
__device__ __forceinline__ void row_times(const double* w, const double (&x)[P], double (&acc)[P], int nx) {
#pragma unroll
    for (int c = 0; c < P; c++) {
        if (c < nx) {
            const double2* row = reinterpret_cast<const double2*>(w + c * LD);
#pragma unroll
            for (int j = 0; j < P; j += 2) {
                const double2 v = row[j / 2];
                acc[j] = fma(x[c], v.x, acc[j]);
                acc[j + 1] = fma(x[c], v.y, acc[j + 1]);
            }
        }
    }
}
// acc_j += sum_{c < nx} T_rc W_cj, c ascending: the multiplier is this lane's row of the panel t (a transposed matrix's column of the original)
template <int P, int LD>
__device__ __forceinline__ void panel_row_times(const double* t, const double* w, int r, double (&acc)[P], int nx) {
#pragma unroll
    for (int c = 0; c < P; c++) {
        if (c < nx) {
            const double x = t[r * LD + c];
            const double2* row = reinterpret_cast<const double2*>(w + c * LD);
#pragma unroll
            for (int j = 0; j < P; j += 2) {
                const double2 v = row[j / 2];
                acc[j] = fma(x, v.x, acc[j]);
                acc[j + 1] = fma(x, v.y, acc[j + 1]);
            }
        }
    }
}
// this lane's row of G0 = (Gam inv(R)) Gam' from its row of Gam and Gam's rows at gp [P x 8]: y_a = sum_b gam_b Rinv_ba, G0_rj = sum_a y_a Gam_ja
template <int P>
__device__ __forceinline__ void g0_row(const DlqrArgs& a, const double* gp, const double (&gam)[DLQR_NU_MAX], double (&g0)[P]) {
    const int nu = a.nu;
    double y[DLQR_NU_MAX];
#pragma unroll
    for (int c = 0; c < DLQR_NU_MAX; c++) {
        double acc = 0.0;
        if (c < nu) {
#pragma unroll
            for (int b = 0; b < DLQR_NU_MAX; b++)
                if (b < nu) acc = fma(gam[b], a.rinv[b * nu + c], acc);
        }
        y[c] = acc;
    }
#pragma unroll
    for (int j = 0; j < P; j++) {
        const double2* row = reinterpret_cast<const double2*>(gp + j * DLQR_NU_MAX);
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < DLQR_NU_MAX; c += 2) {
            const double2 v = row[c / 2];
            if (c < nu) acc = fma(y[c], v.x, acc);
            if (c + 1 < nu) acc = fma(y[c + 1], v.y, acc);
        }
        g0[j] = acc;
    }
}

template <int P>
__global__ __launch_bounds__(DLQR_WAVE) void k_lss_dlqr(DlqrArgs a) {
    using Pan = Panels<P>;
    constexpr int LD = Pan::LD, SLD = Pan::SLD, NG = DLQR_WAVE / P, NU = DLQR_NU_MAX;
    __shared__ __attribute__((aligned(16))) double lds[NG * Pan::GRP];
    const fbg::Lanes<P> g;
    double* mp = lds + (threadIdx.x / P) * Pan::GRP;   // rows of the right factor of a product
    double* tp = mp + P * LD;                          // a transposed matrix; outside the loop also Gam's rows [P x 8]
    double* sol = tp + P * LD;                         // the solve's rows [V | U]; once they are read, K's rows [8 x P]
    double* prow = sol + P * SLD;
    double* gp = tp;
    double* kp = sol;
    const int r = g.r;
    const int nx = a.nx, nu = a.nu, ny = a.ny;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t S = n * a.G, slot0 = i * a.G;
    const bool live = r < nx;

    // ---- A = Phi, H = Q, G = G0
    double am[P], gm[P], hm[P];
    {
        double gam[NU];
#pragma unroll
        for (int c = 0; c < NU; c++) gam[c] = (live && c < nu) ? a.ab[ab_index(S, slot0, a.G + c) + r] : 0.0;
        rows_put<NU, NU>(gp, r, gam);
        g0_row<P>(a, gp, gam, gm);
    }
#pragma unroll
    for (int c = 0; c < P; c++) {
        const bool in = live && c < nx;
        am[c] = in ? a.ab[ab_index(S, slot0, c) + r] : 0.0;
        hm[c] = in ? a.q[r + nx * c] : 0.0;
        gm[c] = in ? gm[c] : 0.0;
    }

    // ---- the doublings: as long as a group of the wave is still running
    int iters = 0, status = 0;
    bool run = true;
#pragma unroll 1
    for (int it = 0; it < FB_DLQR_MAX_ITERS; it++) {
        if (__ballot(run) == 0) break;
        rows_put<P, LD>(mp, r, hm);
        Row<P, 2 * P> w;
#pragma unroll
        for (int c = 0; c < P; c++) { w.e[c] = c == r ? 1.0 : 0.0; w.rhs[c] = am[c]; w.rhs[P + c] = gm[c]; }
        row_times<P, LD>(mp, gm, w.e, nx);
        const Solve sv = gj_solve<P, SLD, P, 2 * P>(g, w, prow, sol, live, nx);
        cols_put<P, LD>(tp, r, am);
        double t[P], hn[P], gn[P];
        // H + A' (H V)
#pragma unroll
        for (int c = 0; c < P; c++) { t[c] = 0.0; hn[c] = hm[c]; gn[c] = gm[c]; }
        row_times<P, SLD>(sol, hm, t, nx);
        rows_put<P, LD>(mp, r, t);
        panel_row_times<P, LD>(tp, mp, r, hn, nx);
        // G + (A U) A'
#pragma unroll
        for (int c = 0; c < P; c++) t[c] = 0.0;
        row_times<P, SLD>(sol + P, am, t, nx);
        row_times<P, LD>(tp, t, gn, nx);
        // A V
#pragma unroll
        for (int c = 0; c < P; c++) t[c] = 0.0;
        row_times<P, SLD>(sol, am, t, nx);
        double dh = 0.0, hmax = 0.0, amax = 0.0;
        bool fin = true;
#pragma unroll
        for (int c = 0; c < P; c++) {
            dh = fmax(dh, fabs(hn[c] - hm[c]));
            hmax = fmax(hmax, fabs(hn[c]));
            amax = fmax(amax, fabs(t[c]));
            fin = fin && is_fin(hn[c]) && is_fin(gn[c]) && is_fin(t[c]);
        }
        dh = g.gmax(live ? dh : 0.0); hmax = g.gmax(live ? hmax : 0.0); amax = g.gmax(live ? amax : 0.0);
        const bool bad = g.any(!sv.ok) || g.any(live && !fin);
        const bool take = run && live;
#pragma unroll
        for (int c = 0; c < P; c++) {
            am[c] = take ? t[c] : am[c];
            gm[c] = take ? gn[c] : gm[c];
            hm[c] = take ? hn[c] : hm[c];
        }
        if (run) {
            iters++;
            if (bad) { status = FB_DLQR_SINGULAR; run = false; }
            else if (dh <= DLQR_TOL * hmax && amax <= DLQR_A_TOL) run = false;
        }
    }
    if (run) status = FB_DLQR_NOT_CONVERGED;

    // ---- X = (H + H') / 2: H's rows into the panel, lane r reads column r
    double x[P];
    bool fin = true;
    double xmax = 0.0;
    rows_put<P, LD>(mp, r, hm);
#pragma unroll
    for (int c = 0; c < P; c++) {
        x[c] = (live && c < nx) ? 0.5 * (hm[c] + mp[c * LD + r]) : 0.0;
        fin = fin && is_fin(x[c]);
        xmax = fmax(xmax, fabs(x[c]));
    }
    // ---- Phic = inv(I + G0 X) Phi
    double gam[NU], phi[P];
#pragma unroll
    for (int c = 0; c < NU; c++) gam[c] = (live && c < nu) ? a.ab[ab_index(S, slot0, a.G + c) + r] : 0.0;
#pragma unroll
    for (int c = 0; c < P; c++) phi[c] = (live && c < nx) ? a.ab[ab_index(S, slot0, c) + r] : 0.0;
    rows_put<NU, NU>(gp, r, gam);
    bool ok3;
    {
        double g0[P];
        g0_row<P>(a, gp, gam, g0);
        rows_put<P, LD>(mp, r, x);
        Row<P, P> w;
#pragma unroll
        for (int c = 0; c < P; c++) { w.e[c] = c == r ? 1.0 : 0.0; w.rhs[c] = phi[c]; }
        row_times<P, LD>(mp, g0, w.e, nx);
        const Solve sv = gj_solve<P, SLD, P, P>(g, w, prow, sol, live, nx);
        ok3 = !g.any(!sv.ok);
    }
    // ---- K = inv(R) (Gam' (X Phic)): lane c has column c
    double t[P];
#pragma unroll
    for (int c = 0; c < P; c++) t[c] = 0.0;
    row_times<P, SLD>(sol, x, t, nx);
    rows_put<P, LD>(mp, r, t);
    double kc[NU];
    {
        double y[NU];
#pragma unroll
        for (int b = 0; b < NU; b++) {
            double acc = 0.0;
            if (b < nu) {
#pragma unroll
                for (int m = 0; m < P; m++)
                    if (m < nx) acc = fma(gp[m * NU + b], mp[m * LD + r], acc);
            }
            y[b] = acc;
        }
#pragma unroll
        for (int c = 0; c < NU; c++) {
            double acc = 0.0;
            if (c < nu) {
#pragma unroll
                for (int b = 0; b < NU; b++)
                    if (b < nu) acc = fma(a.rinv[c * nu + b], y[b], acc);
            }
            kc[c] = live ? acc : 0.0;
            fin = fin && is_fin(kc[c]);
        }
    }
    panel_sync();
#pragma unroll
    for (int c = 0; c < NU; c++) kp[c * P + r] = kc[c];
    panel_sync();
    // ---- Phi - Gam K, and the residual Phi' (X (Phi - Gam K)) - X + Q
    double pcl[P];
#pragma unroll
    for (int c = 0; c < P; c++) pcl[c] = phi[c];
#pragma unroll
    for (int b = 0; b < NU; b++) {
        if (b < nu) {
            const double2* row = reinterpret_cast<const double2*>(kp + b * P);
#pragma unroll
            for (int j = 0; j < P; j += 2) {
                const double2 v = row[j / 2];
                pcl[j] = fma(-gam[b], v.x, pcl[j]);
                pcl[j + 1] = fma(-gam[b], v.y, pcl[j + 1]);
            }
        }
    }
    rows_put<P, LD>(mp, r, pcl);
#pragma unroll
    for (int c = 0; c < P; c++) t[c] = 0.0;
    row_times<P, LD>(mp, x, t, nx);
    cols_put<P, LD>(tp, r, phi);
    rows_put<P, LD>(mp, r, t);
#pragma unroll
    for (int c = 0; c < P; c++) t[c] = 0.0;
    panel_row_times<P, LD>(tp, mp, r, t, nx);
    double rmax = 0.0;
#pragma unroll
    for (int c = 0; c < P; c++) {
        if (live && c < nx) {
            const double e = (t[c] - x[c]) + a.q[r + nx * c];
            rmax = fmax(rmax, fabs(e));
            fin = fin && is_fin(e);
        }
    }
    rmax = g.gmax(rmax); xmax = g.gmax(xmax);
    if (status == 0 && (!ok3 || g.any(!fin))) status = FB_DLQR_SINGULAR;
    if (!valid) return;
    const double nan = __builtin_nan("");
    const bool good = status == 0;
    if (live) {
        if (a.X) {
#pragma unroll
            for (int c = 0; c < P; c++)
                if (c < nx) a.X[staged_index(n, i, nx, r, c)] = good ? x[c] : nan;
        }
        if (a.K) {
#pragma unroll
            for (int b = 0; b < NU; b++)
                if (b < nu) a.K[staged_index(n, i, nu, b, r)] = good ? kc[b] : nan;
        }
    }
    if (r == 0) {
        if (a.resid) a.resid[i] = good ? rmax / fmax(a.qmax, xmax) : nan;
        if (a.iters) a.iters[i] = iters;
        if (a.status) a.status[i] = status;
    }
    if (!a.AB) return;

    // ---- the closed model: [Phi - Gam K | Gam], [C - D K | D], delta, x0, u0 and y0 as they are
    if (live) {
        a.xdot0[(int64_t)r * n + i] = a.xs[slot0 + r];
        a.x0[(int64_t)r * n + i] = a.xs[S + slot0 + r];
#pragma unroll
        for (int c = 0; c < P; c++)
            if (c < nx) a.AB[staged_index(n, i, nx, r, c)] = good ? pcl[c] : nan;
#pragma unroll
        for (int b = 0; b < NU; b++)
            if (b < nu) a.AB[staged_index(n, i, nx, r, nx + b)] = gam[b];
    }
    for (int j = r; j < nu; j += P) a.u0_out[(int64_t)j * n + i] = a.u0[(int64_t)j * n + i];
    for (int j = r; j < ny; j += P) {
        a.y0_out[(int64_t)j * n + i] = a.y0[(int64_t)j * n + i];
        for (int b = 0; b < nu; b++) a.CD[staged_index(n, i, ny, j, nx + b)] = a.cd[cd_index(n, i, ny, j, nx + b)];
        for (int c = 0; c < nx; c++) {
            double v = a.cd[cd_index(n, i, ny, j, c)];
            for (int b = 0; b < nu; b++) v = fma(-a.cd[cd_index(n, i, ny, j, nx + b)], kp[b * P + c], v);
            a.CD[staged_index(n, i, ny, j, c)] = good ? v : nan;
        }
    }
}

}  // namespace fbk
