// surgery_kernels.hpp — design-model surgery for a batch of linear models on the device (include/flightbatch.h: fb_lss_transform,
// fb_lss_steady; host side: fb_surgery.inc; docs/design/linearize.md, "Design-model surgery on the device"; numpy restatement:
// tests/surgery_prototype.py). Reference: get_design_model! (FA design/c172/c172x_design.jl:23-82) and K_fwd = M22 + K M12 with
// M = inv([A B; C D]) (:184-188, :371-381).
//   k_transform  T = C[rows, :];  A' = T A inv(T), B' = T B, C' = C inv(T), D' = D, xdot0' = T xdot0 (masked entries exactly 0), x0' = y0[rows]
//   k_steady     L = [A B; C[iz, :] D[iz, :]];  L [X; U] = [0; I];  K_fwd = U + K X
//                DISC (fb_lss_dsteady, a sampled model): L = [Phi - I, Gamma; C_z D_z], the identity subtracted while the rows are staged;
//                K_fbk = K - Ts K_xi C_z (K_xi given), K_fwd = U + K_fbk X
// One system per group of P lanes of one wave (P = 8, 16 or 32, the smallest with a lane per row of T or of L; 64 / P systems per wave,
// one wave per workgroup). Lane r owns row r of the augmented rows ([T | I], [L | 0; I]) as an fbg::Row; the family's solve
// (fbg::gj_solve, lss_group.hpp: Gauss-Jordan elimination, the rows staying with their lanes) puts row k of the solution
// at row k of the group's LDS panel, from where every product reads it back as broadcasts. Every sum starts from its first term's
// accumulator (0, or U for K_fwd) and runs with k ascending as explicit fma, so a result is a function of the system's own values
// only. The panel belongs to one wave: fences and wave_barrier, no s_barrier. Lanes past the batch's end work on the last system
// again and store nothing. k_transform's result goes to a staging block in fb_linearize's layout; fbl::k_lss_gather makes the new
// handle's copy from it (and applies the subsystem lists). With rows == NULL k_transform copies and does no arithmetic.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbm {

using namespace fbg;

constexpr int SG_WAVE = fbg::WAVE;
constexpr int SG_NU_MAX = 8;      // the inputs of a model: fbl::LSS_NU_MAX

struct TransformArgs {
    const double* ab; const double* xs; const double* u0; const double* y0; const double* cd;   // the source handle's copies (fbg::ab_index)
    int nx, nu, ny, G;
    int64_t n;
    const int32_t* rows;                  // [nx] rows of C that form T; NULL: T = I, a copy
    uint32_t zero;                        // bit r: xdot0'_r is exactly 0
    double *xdot0, *x0, *u0_out, *y0_out; // staging, fb_linearize's layout: vectors [rows x n]
    double* AB; double* CD;               // [(r + nx c) n + i] over nx + nu columns, [(j + ny c) n + i]
    int32_t* status; double* rpiv;
};

struct SteadyArgs {
    const double* ab; const double* cd;
    int nx, nu, ny, G;
    int64_t n;
    const int32_t* iz;                    // [nu] rows of the outputs
    const double* K;                      // element (r, k) at [(r + nu k) k_e + i k_s]: (k_e, k_s) = (1, 0) for the batch's matrix, (n, 1) per system; may be NULL
    int64_t k_e, k_s;
    double *X, *U, *Kfwd;                 // [(r + nx c) n + i], [(r + nu c) n + i] twice; each may be NULL
    int32_t* status; double* rpiv;
    // DISC only: K_xi [nu x nu] by K's rule (may be NULL), the sample time, K_fbk [(r + nu c) n + i] over nx columns (may be NULL)
    const double* Kxi;
    double Ts;
    double* Kfbk;
};

template <int P>
__global__ __launch_bounds__(SG_WAVE) void k_transform(TransformArgs a) {
    constexpr int NW = SG_NU_MAX, LD = P + NW + 1, NG = SG_WAVE / P, ROW = 2 * P, GRP = ROW + P * LD;   // (ROW and GRP are even: 16-byte rows)
    __shared__ __attribute__((aligned(16))) double lds[NG * GRP];
    const fbg::Lanes<P> g;
    double* prow = lds + (threadIdx.x / P) * GRP;   // the scaled pivot row of the current step: e | rhs
    double* sol = prow + ROW;                       // inv(T), then [A inv(T) | B | xdot0]: P x LD
    const int r = g.r;
    const int nx = a.nx, nu = a.nu, ny = a.ny;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t S = n * a.G, slot0 = i * a.G;
    const double* cdp = a.cd + i * ny;              // (j, col) of [C | D] at cdp[col cpitch + j]
    const int64_t cpitch = n * ny;
    const bool live = r < nx;
    const bool zeroed = (a.zero >> r) & 1u;

    // ---- what both paths copy: u0, y0
    if (valid) {
        for (int j = r; j < nu; j += P) a.u0_out[(int64_t)j * n + i] = a.u0[(int64_t)j * n + i];
        for (int j = r; j < ny; j += P) a.y0_out[(int64_t)j * n + i] = a.y0[(int64_t)j * n + i];
    }

    // ---- rows == NULL: the model as it is, entry by entry
    if (!a.rows) {
        if (!valid) return;
        if (live) {
            for (int c = 0; c < nx; c++) a.AB[staged_index(n, i, nx, r, c)] = a.ab[ab_index(S, slot0, c) + r];
            for (int c = 0; c < nu; c++) a.AB[staged_index(n, i, nx, r, nx + c)] = a.ab[ab_index(S, slot0, a.G + c) + r];
            a.xdot0[(int64_t)r * n + i] = zeroed ? 0.0 : a.xs[slot0 + r];
            a.x0[(int64_t)r * n + i] = a.xs[S + slot0 + r];
        }
        for (int j = r; j < ny; j += P)
            for (int c = 0; c < nx + nu; c++) a.CD[staged_index(n, i, ny, j, c)] = cdp[(int64_t)c * cpitch + j];
        if (r == 0) {
            if (a.status) a.status[i] = 0;
            if (a.rpiv) a.rpiv[i] = 1.0;
        }
        return;
    }

    // ---- every entry of the source that the new model is made of
    bool fin = model_finite<P>(a.ab, a.cd, nx, nu, ny, a.G, n, i, r);
    if (live) fin = fin && is_fin(a.xs[slot0 + r]);

    // ---- this lane's row of [T | I]
    const int z = live ? a.rows[r] : 0;
    Row<P, P> tv;                                   // e: T, rhs: I
#pragma unroll
    for (int c = 0; c < P; c++) {
        tv.e[c] = (live && c < nx) ? cdp[(int64_t)c * cpitch + z] : 0.0;
        tv.rhs[c] = (live && c == r) ? 1.0 : 0.0;
    }

    // ---- [. | inv(T)]: row k of inv(T) at row k of sol
    const Solve sv = gj_solve<P, LD>(g, tv, prow, sol, live, nx);

    // ---- the system's status
    const Verdict vd = verdict<P>(g, fin, sv, FB_SURGERY_NOT_FINITE, FB_SURGERY_SINGULAR);
    const bool good = vd.status == 0;
    const double nan = __builtin_nan("");
    if (valid && r == 0) {
        if (a.status) a.status[i] = vd.status;
        if (a.rpiv) a.rpiv[i] = vd.rpiv;
    }

    // ---- rows r, r + P, ... of [C' | D'] = [C inv(T) | D]
    for (int j = r; j < ny; j += P) {
        double cr[P];
#pragma unroll
        for (int c = 0; c < P; c++) cr[c] = 0.0;
        for (int k = 0; k < nx; k++) {
            const double s = cdp[(int64_t)k * cpitch + j];
            const double* w = sol + k * LD;
#pragma unroll
            for (int c = 0; c < P; c++) cr[c] = fma(s, w[c], cr[c]);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < P; c++)
                if (c < nx) a.CD[staged_index(n, i, ny, j, c)] = good ? cr[c] : nan;
            for (int c = 0; c < nu; c++) a.CD[staged_index(n, i, ny, j, nx + c)] = good ? cdp[(int64_t)(nx + c) * cpitch + j] : nan;
        }
    }

    // ---- row r of A inv(T), then the panel holds [A inv(T) | B | xdot0]
    double w[P];
#pragma unroll
    for (int c = 0; c < P; c++) w[c] = 0.0;
    if (live) {
        for (int k = 0; k < nx; k++) {
            const double s = a.ab[ab_index(S, slot0, k) + r];
            const double* q = sol + k * LD;
#pragma unroll
            for (int c = 0; c < P; c++) w[c] = fma(s, q[c], w[c]);
        }
    }
    panel_sync();
    if (live) {
#pragma unroll
        for (int c = 0; c < P; c++) sol[r * LD + c] = w[c];
#pragma unroll
        for (int c = 0; c < NW; c++) sol[r * LD + P + c] = c < nu ? a.ab[ab_index(S, slot0, a.G + c) + r] : 0.0;
        sol[r * LD + P + NW] = a.xs[slot0 + r];
    }
    panel_sync();

    // ---- row r of [A' | B' | xdot0'] = T [A inv(T) | B | xdot0], and x0'
    if (live) {
        double o[LD];
#pragma unroll
        for (int c = 0; c < LD; c++) o[c] = 0.0;
        for (int k = 0; k < nx; k++) {
            const double s = cdp[(int64_t)k * cpitch + z];
            const double* q = sol + k * LD;
#pragma unroll
            for (int c = 0; c < LD; c++) o[c] = fma(s, q[c], o[c]);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < P; c++)
                if (c < nx) a.AB[staged_index(n, i, nx, r, c)] = good ? o[c] : nan;
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nu) a.AB[staged_index(n, i, nx, r, nx + c)] = good ? o[P + c] : nan;
            a.xdot0[(int64_t)r * n + i] = good ? (zeroed ? 0.0 : o[P + NW]) : nan;
            a.x0[(int64_t)r * n + i] = a.y0[(int64_t)z * n + i];
        }
    }
}

// the body of k_steady (DISC = false) and of fbj::k_dsteady (DISC = true, dtracker_kernels.hpp): one statement of the map for both times
template <int P, bool DISC>
__device__ __forceinline__ void steady_body(const SteadyArgs& a) {
    constexpr int NW = SG_NU_MAX, LD = NW + 1, NG = SG_WAVE / P, ROW = P + NW, GRP = ROW + P * LD;   // (ROW and GRP are even: 16-byte rows)
    __shared__ __attribute__((aligned(16))) double lds[NG * GRP];
    const fbg::Lanes<P> g;
    double* prow = lds + (threadIdx.x / P) * GRP;   // the scaled pivot row of the current step: e | rhs
    double* sol = prow + ROW;                       // [X; U], P x LD
    const int r = g.r;
    const int nx = a.nx, nu = a.nu, ny = a.ny, m = nx + nu;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t S = n * a.G, slot0 = i * a.G;
    const bool live = r < m, top = r < nx;

    // ---- this lane's row of [L | 0; I]: rows of [A | B], then rows iz of [C | D]
    const int z = (live && !top) ? a.iz[r - nx] : 0;
    const double* src = top ? a.ab + slot0 + r : a.cd + cd_index(n, i, ny, z, 0);
    const int64_t pitch = top ? S : n * ny;
    bool fin = true;
    Row<P, NW> lr;                                  // e: L, rhs: [0; I]
#pragma unroll
    for (int c = 0; c < P; c++) {
        double e = 0.0;
        if (live && c < m) e = src[(int64_t)((top && c >= nx) ? a.G + c - nx : c) * pitch];
        fin = fin && is_fin(e);
        if constexpr (DISC) { if (top && c == r) e -= 1.0; }
        lr.e[c] = e;
    }
#pragma unroll
    for (int c = 0; c < NW; c++) lr.rhs[c] = (live && r == nx + c) ? 1.0 : 0.0;
    if (a.K && r < nu)
        for (int k = 0; k < nx; k++) fin = fin && is_fin(a.K[((int64_t)r + (int64_t)nu * k) * a.k_e + i * a.k_s]);
    // DISC with K_xi: its entries, and whether D_z has a non-zero entry (the lanes of the rows of [C_z | D_z] look at their own)
    bool direct = false;
    if constexpr (DISC) {
        if (a.Kxi) {
            if (r < nu)
                for (int k = 0; k < nu; k++) fin = fin && is_fin(a.Kxi[((int64_t)r + (int64_t)nu * k) * a.k_e + i * a.k_s]);
            bool dnz = false;
#pragma unroll
            for (int c = 0; c < P; c++) dnz = dnz || (live && !top && c >= nx && lr.e[c] != 0.0);
            direct = g.any(dnz);
        }
    }

    // ---- [. | X; U]: row k of [X; U] at row k of sol
    const Solve sv = gj_solve<P, LD>(g, lr, prow, sol, live, m);

    Verdict vd = verdict<P>(g, fin, sv, FB_SURGERY_NOT_FINITE, FB_SURGERY_SINGULAR);
    const bool good = vd.status == 0;
    if (good && direct) vd.status = FB_DSTEADY_DIRECT;   // (X and U are delivered; K_fbk and K_fwd are not)
    const bool gains = vd.status == 0;
    const double nan = __builtin_nan("");
    if (valid && r == 0) {
        if (a.status) a.status[i] = vd.status;
        if (a.rpiv) a.rpiv[i] = vd.rpiv;
    }

    // ---- row r of X (r < nx) or row r - nx of U
    if (live && valid) {
        double* out = top ? a.X : a.U;
        const int rows = top ? nx : nu, ro = top ? r : r - nx;
        if (out) {
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nu) out[staged_index(n, i, rows, ro, c)] = good ? sol[r * LD + c] : nan;
        }
    }
    // ---- row r of K_fwd = U + K X (DISC: of K_fbk = K - Ts K_xi C_z, and K_fwd = U + K_fbk X)
    if (a.K && (a.Kfwd || (DISC && a.Kfbk)) && r < nu) {
        double acc[NW];
#pragma unroll
        for (int c = 0; c < NW; c++) acc[c] = sol[(nx + r) * LD + c];
        for (int k = 0; k < nx; k++) {
            double kk = a.K[((int64_t)r + (int64_t)nu * k) * a.k_e + i * a.k_s];
            if constexpr (DISC) {
                if (a.Kxi) {
                    double s = 0.0;
                    for (int c = 0; c < nu; c++)
                        s = fma(a.Kxi[((int64_t)r + (int64_t)nu * c) * a.k_e + i * a.k_s], a.cd[cd_index(n, i, ny, a.iz[c], k)], s);
                    kk = fma(-a.Ts, s, kk);
                }
                if (a.Kfbk && valid) a.Kfbk[staged_index(n, i, nu, r, k)] = gains ? kk : nan;
            }
            const double* q = sol + k * LD;
#pragma unroll
            for (int c = 0; c < NW; c++) acc[c] = fma(kk, q[c], acc[c]);
        }
        if (valid && a.Kfwd) {
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nu) a.Kfwd[staged_index(n, i, nu, r, c)] = gains ? acc[c] : nan;
        }
    }
}

template <int P>
__global__ __launch_bounds__(SG_WAVE) void k_steady(SteadyArgs a) { steady_body<P, false>(a); }

}  // namespace fbm
