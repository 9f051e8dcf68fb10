// c2d_kernels.hpp — zero-order-hold discretisation of a batch of linear models on the device (include/flightbatch.h: fb_lss_c2d; host side:
// fb_c2d.inc; docs/design/linearize.md, "Sampled models on the device"; numpy restatement, operation for operation: tests/c2d_prototype.py).
// Reference: the exact samples of ControlSystems' step(T, t_sim) (FA design/pidopt.jl, design/robot2d/robot2d_design.ipynb) and
// lsim(e2q, (x, t) -> [0.1] * (t >= 1), 0:0.01:10) (demos/c172_demos.jl); the algorithm is ours.
//   the map   Psi = int_0^Ts e^(A tau) dtau,  Phi = e^(A Ts) = I + A Psi,  Gamma = Psi B,  delta = Psi xdot0:
//             x+ = x0 + Phi (x - x0) + Gamma (u - u0) + delta. A is never inverted (an integrator in series makes it singular).
//   scaling   s = the smallest integer >= 0 with |A|_inf Ts / 2^s <= 1/2 (|A|_inf: the group maximum of each lane's absolute row sum,
//             columns ascending), h = Ts / 2^s, Z = A h
//   Horner    S = I + Z/2 (I + Z/3 (... (I + Z/(m + 1)))), m = C2D_DEG, from S = I: S <- I + (Z S) r_k, r_k = 1 / (k + 1), k = m .. 1
//             (Psi_h = h S);  T = (S W) h with W = [B | xdot0], the thin block;  Phi = I + Z S
//   squaring  s times: T <- T + Phi T, then Phi <- Phi Phi.  Gamma | delta = T.
// The thin form: the squarings carry T = Psi [B | xdot0] (C2D_NB = 10 columns: B's 8, zero past nu, xdot0, one of padding) instead of the
// full Psi, which nothing reads once Gamma and delta are known: a squaring is P^2 (P + 10) instead of 2 P^3 products per group, and the
// 32-lane instance holds two full rows and a thin one in registers instead of three full rows.
//
// k_lss_c2d: one system per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx; 64 / P systems per wave, one wave per
// workgroup); lane r owns row r of every matrix. A product X W keeps X's row in registers; W's rows are published in the group's LDS panel
// and read back as 16-byte broadcasts, every sum an explicit fma with the columns ascending, so a result is a function of the system's own
// values only. Rows r >= nx are those of the identity (Z's are zero) and columns c >= nx of the rows r < nx stay exact zeros. The groups of
// a wave square a different number of times: the loop runs wave_max(s) times behind a wave-uniform bound and a group whose own s is
// exhausted keeps its values. The panel belongs to one wave: fences and wave_barrier, no workgroup barrier. Lanes past the batch's end work on the last
// system again and store nothing. The result goes to a staging block in fb_linearize's layout; fbl::k_lss_gather makes the new handle's
// copy from it.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbz {

using namespace fbg;

constexpr int C2D_WAVE = fbg::WAVE;
constexpr int C2D_DEG = 16;       // m: |Z|_inf <= 1/2, so the first term left out is below 2^-17 / 18! of the sum
constexpr int C2D_NU_MAX = 8;     // the inputs of a model: fbl::LSS_NU_MAX
constexpr int C2D_NB = C2D_NU_MAX + 2;   // columns of the thin block: B | xdot0 | 0 (even: 16-byte reads)

// r_k = 1 / (k + 1), correctly rounded (folded when this is compiled: no reciprocal approximation at run time)
__constant__ double C2D_RK[C2D_DEG + 1] = {1.0, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5, 1.0 / 6, 1.0 / 7, 1.0 / 8, 1.0 / 9, 1.0 / 10, 1.0 / 11,
                                           1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16, 1.0 / 17};

struct C2dArgs {
    const double* ab; const double* xs; const double* u0; const double* y0; const double* cd;   // the source handle's copies (fbg::ab_index)
    int nx, nu, ny, G;
    int64_t n;
    double Ts;
    double *xdot0, *x0, *u0_out, *y0_out; // staging, fb_linearize's layout: vectors [rows x n]; xdot0 takes delta
    double* AB; double* CD;               // [Phi | Gamma] at [(r + nx c) n + i] over nx + nu columns, [C | D] at [(j + ny c) n + i]
    int32_t* squarings; int32_t* status;  // [n]
};

// acc_j += sum_c x_c W_cj, c ascending: W's rows [P x NC] in the group's panel, read as 16-byte broadcasts
template <int P, int NC>
__device__ __forceinline__ void row_times(const double* w, const double (&x)[P], double (&acc)[NC]) {
#pragma unroll
    for (int c = 0; c < P; c++) {
        const double2* row = reinterpret_cast<const double2*>(w + c * NC);
#pragma unroll
        for (int j = 0; j < NC; j += 2) {
            const double2 v = row[j / 2];
            acc[j] = fma(x[c], v.x, acc[j]);
            acc[j + 1] = fma(x[c], v.y, acc[j + 1]);
        }
    }
}
// this lane's row of W into the group's panel, once the reads of what it held are done; readable when this returns
template <int NC>
__device__ __forceinline__ void publish(double* w, int r, const double (&row)[NC]) {
    panel_sync();
#pragma unroll
    for (int c = 0; c < NC; c++) w[r * NC + c] = row[c];
    panel_sync();
}

template <int P>
__global__ __launch_bounds__(C2D_WAVE) void k_lss_c2d(C2dArgs a) {
    constexpr int NB = C2D_NB, NG = C2D_WAVE / P, GRP = P * P + P * NB;   // (GRP, P and NB are even: 16-byte rows)
    __shared__ __attribute__((aligned(16))) double lds[NG * GRP];
    const fbg::Lanes<P> g;
    double* mat = lds + (threadIdx.x / P) * GRP;    // a full factor's rows: P x P
    double* thin = mat + P * P;                     // the thin block's rows: P x NB
    const int r = g.r;
    const int nx = a.nx, nu = a.nu, ny = a.ny;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t S = n * a.G, slot0 = i * a.G;
    const bool live = r < nx;

    // ---- what is copied bit for bit: x0, u0, y0, [C | D]
    if (valid) {
        if (live) a.x0[(int64_t)r * n + i] = a.xs[S + slot0 + r];
        for (int j = r; j < nu; j += P) a.u0_out[(int64_t)j * n + i] = a.u0[(int64_t)j * n + i];
        for (int j = r; j < ny; j += P) {
            a.y0_out[(int64_t)j * n + i] = a.y0[(int64_t)j * n + i];
            for (int c = 0; c < nx + nu; c++) a.CD[staged_index(n, i, ny, j, c)] = a.cd[cd_index(n, i, ny, j, c)];
        }
    }

    // ---- this lane's row of A and of W = [B | xdot0 | 0]; the row sum, whether every entry is finite
    double z[P], w0[NB];
    bool fin = true;
    double rs = 0.0;
#pragma unroll
    for (int c = 0; c < P; c++) {
        z[c] = (live && c < nx) ? a.ab[ab_index(S, slot0, c) + r] : 0.0;
        fin = fin && is_fin(z[c]);
        rs = rs + fabs(z[c]);
    }
#pragma unroll
    for (int c = 0; c < C2D_NU_MAX; c++) w0[c] = (live && c < nu) ? a.ab[ab_index(S, slot0, a.G + c) + r] : 0.0;
    w0[C2D_NU_MAX] = live ? a.xs[slot0 + r] : 0.0;
    w0[C2D_NU_MAX + 1] = 0.0;
#pragma unroll
    for (int c = 0; c < NB; c++) fin = fin && is_fin(w0[c]);
    const bool bad_in = g.any(!fin);

    // ---- s and h = Ts / 2^s (halving is exact); s stops one past FB_C2D_SQUARINGS_MAX
    int s = 0;
    double h = a.Ts;
    {
        double v = g.gmax(rs) * a.Ts;
#pragma unroll 1
        for (int k = 0; k <= FB_C2D_SQUARINGS_MAX; k++) {
            const bool more = v > 0.5;
            v = more ? 0.5 * v : v;
            h = more ? 0.5 * h : h;
            s = more ? s + 1 : s;
        }
    }
    const bool range = s > FB_C2D_SQUARINGS_MAX;
    const int s_own = (bad_in || range) ? 0 : s;
#pragma unroll
    for (int c = 0; c < P; c++) z[c] = z[c] * h;

    // ---- S by Horner, from S = I
    double sm[P];
#pragma unroll
    for (int c = 0; c < P; c++) sm[c] = c == r ? 1.0 : 0.0;
#pragma unroll 1
    for (int k = C2D_DEG; k >= 1; k--) {
        const double rk = C2D_RK[k];
        publish<P>(mat, r, sm);
#pragma unroll
        for (int c = 0; c < P; c++) sm[c] = 0.0;
        row_times<P, P>(mat, z, sm);
#pragma unroll
        for (int c = 0; c < P; c++) sm[c] = fma(sm[c], rk, c == r ? 1.0 : 0.0);
    }

    // ---- T = (S W) h, then Phi = I + Z S
    double t[NB], phi[P];
    publish<NB>(thin, r, w0);
#pragma unroll
    for (int c = 0; c < NB; c++) t[c] = 0.0;
    row_times<P, NB>(thin, sm, t);
#pragma unroll
    for (int c = 0; c < NB; c++) t[c] = t[c] * h;
    publish<P>(mat, r, sm);
#pragma unroll
    for (int c = 0; c < P; c++) phi[c] = c == r ? 1.0 : 0.0;
    row_times<P, P>(mat, z, phi);

    // ---- the squarings: as many rounds as the wave's slowest group needs
    const int rounds = wave_max<P>(s_own);
#pragma unroll 1
    for (int it = 0; it < rounds; it++) {
        publish<NB>(thin, r, t);
        publish<P>(mat, r, phi);
        double tn[NB], pn[P];
#pragma unroll
        for (int c = 0; c < NB; c++) tn[c] = t[c];
        row_times<P, NB>(thin, phi, tn);
#pragma unroll
        for (int c = 0; c < P; c++) pn[c] = 0.0;
        row_times<P, P>(mat, phi, pn);
        const bool act = it < s_own;
#pragma unroll
        for (int c = 0; c < NB; c++) t[c] = act ? tn[c] : t[c];
#pragma unroll
        for (int c = 0; c < P; c++) phi[c] = act ? pn[c] : phi[c];
    }

    // ---- the system's status: a non-finite input first, then the range, then an overflow
    bool rfin = true;
#pragma unroll
    for (int c = 0; c < P; c++) rfin = rfin && is_fin(phi[c]);
#pragma unroll
    for (int c = 0; c < NB; c++) rfin = rfin && is_fin(t[c]);
    const bool bad_out = g.any(!rfin);
    const int32_t st = bad_in ? FB_C2D_NOT_FINITE : range ? FB_C2D_RANGE : bad_out ? FB_C2D_NOT_FINITE : 0;
    if (!valid) return;
    if (r == 0) {
        a.status[i] = st;
        a.squarings[i] = st ? 0 : s;
    }
    if (!live) return;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < P; c++)
        if (c < nx) a.AB[staged_index(n, i, nx, r, c)] = st ? nan : phi[c];
#pragma unroll
    for (int c = 0; c < C2D_NU_MAX; c++)
        if (c < nu) a.AB[staged_index(n, i, nx, r, nx + c)] = st ? nan : t[c];
    a.xdot0[(int64_t)r * n + i] = st ? nan : t[C2D_NU_MAX];
}

}  // namespace fbz
