// lqr_kernels.hpp — lqr(P, Q, R) for a batch of LinearizedSS models on the device (include/flightbatch.h: fb_lqr; host side: fb_lqr.inc;
// docs/design/linearize.md, "LQR design on the device"; numpy restatement: tests/lqr_prototype.py).
//   H = [[A, -G], [-Q, -A']], G = B inv(R) B';  Z <- (c Z + inv(Z) / c) / 2 with c = |det Z|^(-1 / 2nx) until max|dZ| <= 1e-13 max|Z| (at most
//   LQR_MAX_ITERS times): Z -> W = sign(H);  X = -W21 inv(I - W11), symmetrised;  K = inv(R) B' X.
// One system per group of P lanes of one wave (P = 8, 16 or 32, the smallest with P >= 2 nx; 64 / P systems per wave, one wave per workgroup);
// lane r owns row r of Z. With h = P / 2 the four blocks of H sit at fixed register offsets: rows and columns [0, nx) and [h, h + nx) are the
// Hamiltonian, the others are padding (diagonal -1, held; never a pivot, so not in the determinant; the live rows' padding columns stay 0).
//
// inv(Z): in-place Gauss-Jordan elimination, every step k a compile-time k (the row is a register array). Pivot of step k: the family's rule
// on |Z_ik| (fbg::Lanes::pivot, lss_group.hpp). The rows stay with their lanes (implicit pivoting): with sigma(k) the pivot lane of step k the elimination leaves
// S[sigma(i)][j] = inv(Z)[i][sigma(j)], which one pass through the group's LDS panel undoes. The pivot lane publishes its scaled row in that
// panel and every lane reads it back as P / 2 16-byte broadcasts. The panel belongs to one wave: fences and wave_barrier, no s_barrier.
// Lanes past the batch's end design the last system again and store nothing, so a wave never diverges on the batch size.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbq {

using namespace fbg;

constexpr int LQR_WAVE = fbg::WAVE;
constexpr int LQR_NU_MAX = 8;
constexpr int LQR_MAX_ITERS = 50;
constexpr double LQR_TOL = 1e-13;

struct LqrArgs {
    const double* ab;      // the handle's [A | B] (fbg::ab_index, lss_group.hpp), with its group size G
    const double* q;       // Q, nx x nx column-major (symmetric)
    double *K, *X, *resid; // outputs in fb_linearize's layout, any may be null
    int32_t *iters, *status;
    int64_t n;
    int nx, nu, G;
    double qmax;           // max|Q|
    double rinv[LQR_NU_MAX * LQR_NU_MAX];   // inv(R), element (a, b) at [a nu + b] (symmetric)
};

// the lane group with the LDS panels of k_lqr and k_lss_freqresp
template <int P>
struct Group : fbg::Lanes<P> {
    static constexpr int h = P / 2, LD = P + 1;   // (an odd row pitch: a lane per row or a lane per column, neither collides on a bank)
    static constexpr int PANEL = P * LD, SIDE = LQR_NU_MAX * h;
    double* pan;    // P x LD
    double* ya;     // nu x h: scratch matrices of the prologue and epilogue, (a, c) at [a h + c]
    double* kb;
    int* sig;       // sigma
    __device__ Group(double* lds_d, int* lds_i) {
        const int g = threadIdx.x / P;
        pan = lds_d + g * (PANEL + 2 * SIDE); ya = pan + PANEL; kb = ya + SIDE;
        sig = lds_i + g * P;
    }
};

// w <- inv(w) over the live rows and columns k < KL with k % h < nx (`live`: this lane owns such a row); logdet += sum log|pivot|.
// Returns false when a pivot was zero or not finite (the arithmetic goes on, on whatever that leaves: nothing here can trap or wait).
template <int P, int KL>
__device__ inline bool gj_inverse(double (&w)[P], const Group<P>& g, bool live, int nx, double& logdet) {
    constexpr int h = P / 2, LD = P + 1;
    bool used = !live, ok = true;
    int myk = g.r;
    panel_sync();
    g.sig[g.r] = g.r;
#pragma unroll
    for (int k = 0; k < KL; k++) {
        if (k % h < nx) {
            const Pivot pv = g.pivot(used, used ? -1.0 : fabs(w[k]), k);
            ok = ok && pv.found;
            panel_sync();
            if (g.r == pv.p) {
                const double ip = 1.0 / w[k];
#pragma unroll
                for (int j = 0; j < P; j++) w[j] = j == k ? ip : w[j] * ip;
#pragma unroll
                for (int j = 0; j < P; j++) g.pan[j] = w[j];
                g.sig[k] = g.r;
                used = true; myk = k;
            }
            panel_sync();
            if (g.r != pv.p) {
                const double f = w[k];
                const double2* row = reinterpret_cast<const double2*>(g.pan);
#pragma unroll
                for (int j = 0; j < P; j += 2) {
                    const double2 s = row[j / 2];
                    w[j] = j == k ? -f * s.x : fma(-f, s.x, w[j]);
                    w[j + 1] = j + 1 == k ? -f * s.y : fma(-f, s.y, w[j + 1]);
                }
            }
            logdet += log(pv.m);
        }
    }
    // S[sigma(i)][j] -> inv[i][sigma(j)]
    panel_sync();
#pragma unroll
    for (int j = 0; j < P; j++) g.pan[myk * LD + g.sig[j]] = w[j];
    panel_sync();
#pragma unroll
    for (int j = 0; j < P; j++) w[j] = g.pan[g.r * LD + j];
    return ok;
}

template <int P>
__global__ __launch_bounds__(LQR_WAVE) void k_lqr(LqrArgs a) {
    using Grp = Group<P>;
    constexpr int h = P / 2, LD = P + 1, NG = LQR_WAVE / P;
    __shared__ __attribute__((aligned(16))) double lds_d[NG * (Grp::PANEL + 2 * Grp::SIDE)];
    __shared__ int lds_i[LQR_WAVE];
    const Grp g(lds_d, lds_i);
    const int r = g.r, rr = r % h, nx = a.nx, nu = a.nu;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < a.n;
    const int64_t i = valid ? i_own : a.n - 1;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const bool top = r < h, act = rr < nx, tact = top && act;

    // ---- H: G = B inv(R) B' through the side panels (kb: B', ya: inv(R) B')
    if (tact) {
        for (int b = 0; b < nu; b++) g.kb[b * h + r] = a.ab[ab_index(S, slot0, a.G + b) + r];
    }
    panel_sync();
    if (tact) {
        for (int c = 0; c < nu; c++) {
            double acc = 0.0;
            for (int b = 0; b < nu; b++) acc = fma(a.rinv[c * nu + b], g.kb[b * h + r], acc);
            g.ya[c * h + r] = acc;
        }
    }
    panel_sync();
    double z[P];
#pragma unroll
    for (int c = 0; c < P; c++) z[c] = 0.0;
    if (!act) {
#pragma unroll
        for (int c = 0; c < P; c++) z[c] = c == r ? -1.0 : 0.0;
    } else if (top) {
#pragma unroll
        for (int c = 0; c < h; c++) {
            if (c < nx) {
                z[c] = a.ab[ab_index(S, slot0, c) + r];
                double acc = 0.0;
                for (int b = 0; b < nu; b++) acc = fma(g.ya[b * h + r], g.kb[b * h + c], acc);
                z[h + c] = -acc;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < h; c++) {
            if (c < nx) {
                z[c] = -a.q[rr + nx * c];
                z[h + c] = -a.ab[ab_index(S, slot0, rr) + c];
            }
        }
    }

    // ---- sign(H)
    int iters = 0, status = 0;
    bool run = true;
    const double expo = -1.0 / (double)(2 * nx);
#pragma unroll 1
    for (int it = 0; it < LQR_MAX_ITERS; it++) {
        if (__ballot(run) == 0) break;
        double w[P];
#pragma unroll
        for (int c = 0; c < P; c++) w[c] = z[c];
        double logdet = 0.0;
        const bool ok = gj_inverse<P, P>(w, g, act, nx, logdet);
        const double c = exp(logdet * expo), ci = 1.0 / c;
        double dmax = 0.0, zmax = 0.0;
        bool fin = true;
#pragma unroll
        for (int j = 0; j < P; j++) {
            const double zn = 0.5 * (c * z[j] + ci * w[j]);
            w[j] = zn;
            if (act) {
                dmax = fmax(dmax, fabs(zn - z[j]));
                zmax = fmax(zmax, fabs(zn));
                fin = fin && is_fin(zn);
            }
        }
        dmax = g.gmax(dmax); zmax = g.gmax(zmax);
        const bool bad = !ok || g.any(!fin);
        const bool take = run && act;
#pragma unroll
        for (int j = 0; j < P; j++) z[j] = take ? w[j] : z[j];
        if (run) {
            iters++;
            if (bad) { status = FB_LQR_SINGULAR; run = false; }
            else if (dmax <= LQR_TOL * zmax) run = false;
        }
    }
    if (run) status = FB_LQR_NOT_CONVERGED;

    // ---- X = -W21 inv(I - W11): the elimination once more on the top rows, then the bottom rows times the panel
    double w[P];
#pragma unroll
    for (int c = 0; c < P; c++) w[c] = (c < h && tact && c < nx) ? (c == r ? 1.0 : 0.0) - z[c] : 0.0;
    double unused = 0.0;
    const bool ok3 = gj_inverse<P, h>(w, g, tact, nx, unused);
    panel_sync();
    if (tact) {
#pragma unroll
        for (int c = 0; c < h; c++) g.pan[r * LD + c] = w[c];
    }
    panel_sync();
    double x[h];
#pragma unroll
    for (int c = 0; c < h; c++) x[c] = 0.0;
#pragma unroll
    for (int m = 0; m < h; m++) {
        if (m < nx) {
#pragma unroll
            for (int c = 0; c < h; c++) x[c] = fma(-z[m], g.pan[m * LD + c], x[c]);
        }
    }
    panel_sync();
    if (!top && act) {
#pragma unroll
        for (int c = 0; c < h; c++) g.pan[rr * LD + c] = x[c];
    }
    panel_sync();
    // from here on the top lanes: lane r holds row r of the symmetrised X
    bool fin = true;
    double xmax = 0.0;
#pragma unroll
    for (int c = 0; c < h; c++) {
        x[c] = (tact && c < nx) ? 0.5 * (g.pan[r * LD + c] + g.pan[c * LD + r]) : 0.0;
        fin = fin && is_fin(x[c]);
        xmax = fmax(xmax, fabs(x[c]));
    }
    // Y = B' X (ya) and K = inv(R) Y (kb): lane c has column c of both (X is symmetric: column c of X is this lane's row)
    panel_sync();
    if (tact) {
        for (int b = 0; b < nu; b++) {
            const double* bcol = a.ab + ab_index(S, slot0, a.G + b);
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < h; m++)
                if (m < nx) acc = fma(bcol[m], x[m], acc);
            g.ya[b * h + r] = acc;
        }
        for (int c = 0; c < nu; c++) {
            double acc = 0.0;
            for (int b = 0; b < nu; b++) acc = fma(a.rinv[c * nu + b], g.ya[b * h + r], acc);
            g.kb[c * h + r] = acc;
            fin = fin && is_fin(acc);
        }
    }
    // the residual A'X + XA - Y'K + Q = T + T' - Y'K + Q with T = XA: A's rows into the panel, T's rows back into it
    if (tact) {
#pragma unroll
        for (int c = 0; c < h; c++)
            if (c < nx) g.pan[r * LD + c] = a.ab[ab_index(S, slot0, c) + r];
    }
    panel_sync();
    double t[h];
#pragma unroll
    for (int c = 0; c < h; c++) t[c] = 0.0;
#pragma unroll
    for (int m = 0; m < h; m++) {
        if (m < nx) {
#pragma unroll
            for (int c = 0; c < h; c++) t[c] = fma(x[m], g.pan[m * LD + c], t[c]);
        }
    }
    panel_sync();
    if (tact) {
#pragma unroll
        for (int c = 0; c < h; c++) g.pan[r * LD + c] = t[c];
    }
    panel_sync();
    double rmax = 0.0;
    if (tact) {
#pragma unroll
        for (int c = 0; c < h; c++) {
            if (c < nx) {
                double e = (t[c] + g.pan[c * LD + r]) + a.q[r + nx * c];
                for (int b = 0; b < nu; b++) e = fma(-g.ya[b * h + r], g.kb[b * h + c], e);
                rmax = fmax(rmax, fabs(e));
                fin = fin && is_fin(e);
            }
        }
    }
    rmax = g.gmax(rmax); xmax = g.gmax(xmax);
    if (status == 0 && (!ok3 || g.any(!fin))) status = FB_LQR_SINGULAR;
    if (!valid) return;
    const double nan = __builtin_nan("");
    const bool good = status == 0;
    if (tact) {
        if (a.X) {
#pragma unroll
            for (int c = 0; c < h; c++)
                if (c < nx) a.X[staged_index(a.n, i, nx, r, c)] = good ? x[c] : nan;
        }
        if (a.K) {
            for (int b = 0; b < nu; b++) a.K[staged_index(a.n, i, nu, b, r)] = good ? g.kb[b * h + r] : nan;
        }
    }
    if (r == 0) {
        if (a.resid) a.resid[i] = good ? rmax / fmax(a.qmax, xmax) : nan;
        if (a.iters) a.iters[i] = iters;
        if (a.status) a.status[i] = status;
    }
}

}  // namespace fbq
