// connect_kernels.hpp — connect / series / feedback for a batch of linear models on the device (include/flightbatch.h: fb_lss_connect; host
// side: fb_connect.inc; docs/design/linearize.md, "Closing loops on the device"; numpy restatement: tests/connect_prototype.py).
// Reference: the `connect`, `series` and `feedback` calls of FA design/c172/c172x_design.jl and design/robot2d/robot2d_design.ipynb.
//   plant p (nx_p, nu_p, ny_p), compensator c (nx_c, nu_c, ny_c, may be absent), both in deviation coordinates; v = [u_p; u_c], z = [y_p; y_c],
//   x = [x_p; x_c]; the stacked model x' = A x + B v, z = C x + D v is block-diagonal. Interconnection v = F z[jz] + G w, outputs z[iz]:
//   E = inv(I - F D[jz, :]), M = E F C[jz, :], Nw = E G;  A' = A + B M, B' = B Nw, C' = C[iz, :] + D[iz, :] M, D' = D[iz, :] Nw.
// One system per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= max(nx_p + nx_c, nv); 64 / P systems per wave, one wave per
// workgroup). Lane r < nv owns row r of [I - F D_jz | F C_jz | G] as three register arrays; Gauss-Jordan elimination on the augmented rows,
// the family's solve (fbg::gj_solve, lss_group.hpp) written out here: through the helper k_connect<8> is 2 % slower than it was
// (profiles/lss_solve_refactor.txt). The rows stay with their lanes: the lane that was the pivot of step k ends
// with row k of [M | Nw] and puts it at row k of the group's LDS panel. Lane r < nx then forms row r of [A' | B'], and every lane the output
// rows r, r + P, ... of [C' | D'], reading [M | Nw] back as broadcasts. The blocks of the stacked model that are zero by construction are
// skipped, not multiplied; every sum runs with k ascending as explicit fma, so a result is a function of the system's own values only.
// The panel belongs to one wave: fences and wave_barrier, no s_barrier. Lanes past the batch's end work on the last system again and store
// nothing. The result goes to a staging block in fb_linearize's layout; fbl::k_lss_gather makes the new handle's copy from it.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbc {

using namespace fbg;

constexpr int CN_WAVE = fbg::WAVE;
constexpr int CN_NW_MAX = 8;      // the inputs of the new model: fbl::LSS_NU_MAX

struct ConnectSide {
    const double* ab; const double* cd;   // a handle's copies (fbg::ab_index, lss_group.hpp), G its group size
    int nx, nu, ny, G;
};
struct ConnectArgs {
    ConnectSide p, c;                     // c: all sizes 0 when there is no compensator
    const int32_t* jz; const int32_t* iz; // [nf], [ny]: rows of z
    const double* F; const double* G;     // element (r, k) at [(r + nv k) fe + i fs]: (fe, fs) = (1, 0) for the batch's matrix, (n, 1) per system
    int64_t f_e, f_s, g_e, g_s;
    double* AB; double* CD;               // staging, fb_linearize's layout: [(r + nx c) n + i] over nx + nw columns, [(j + ny c) n + i]
    int32_t* status;
    int64_t n;
    int nf, nw, ny;
};

template <int P>
__global__ __launch_bounds__(CN_WAVE) void k_connect(ConnectArgs a) {
    constexpr int NVP = P < FB_CONNECT_NV_MAX ? P : FB_CONNECT_NV_MAX, NW = CN_NW_MAX;
    constexpr int ROW = NVP + P + NW, LD = P + NW + 1, NG = CN_WAVE / P, GRP = ROW + NVP * LD;   // (ROW and GRP are even: 16-byte rows)
    __shared__ __attribute__((aligned(16))) double lds[NG * GRP];
    const fbg::Lanes<P> g;
    double* prow = lds + (threadIdx.x / P) * GRP;   // the scaled pivot row of the current step: e | m | gw
    double* sol = prow + ROW;                       // [M | Nw], NVP x LD
    const int r = g.r;
    const int nxp = a.p.nx, nup = a.p.nu, nyp = a.p.ny, nxc = a.c.nx, nuc = a.c.nu;
    const int nx = nxp + nxc, nv = nup + nuc, nf = a.nf, nw = a.nw, ny = a.ny;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t Sp = n * a.p.G, slotp = i * a.p.G, Sc = n * a.c.G, slotc = i * a.c.G;
    // cd_index at unrolled columns, base and column pitch hoisted by hand (58 to 185 registers fewer): (z, col) at cdp[col cpitch + z]
    const double* cdp = a.p.cd + i * nyp;
    const double* cdc = a.c.cd + i * a.c.ny;
    const int64_t cpitch = n * nyp, ccpitch = n * a.c.ny;

    // ---- every entry of the sources
    bool fin = model_finite<P>(a.p.ab, a.p.cd, nxp, nup, nyp, a.p.G, n, i, r);
    if (nxc > 0) fin = fin && model_finite<P>(a.c.ab, a.c.cd, nxc, nuc, a.c.ny, a.c.G, n, i, r);

    // ---- this lane's row of [I - F D_jz | F C_jz | G]
    const bool live = r < nv;
    double e[NVP], m[P], gw[NW];
#pragma unroll
    for (int c = 0; c < NVP; c++) e[c] = (live && c == r) ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < P; c++) m[c] = 0.0;
#pragma unroll
    for (int c = 0; c < NW; c++) gw[c] = 0.0;
    if (live) {
        for (int k = 0; k < nf; k++) {
            const int z = a.jz[k];
            const double f = a.F[((int64_t)r + (int64_t)nv * k) * a.f_e + i * a.f_s];
            fin = fin && is_fin(f);
            if (z < nyp) {
#pragma unroll
                for (int c = 0; c < P; c++)
                    if (c < nxp) m[c] = fma(f, cdp[(int64_t)c * cpitch + z], m[c]);
#pragma unroll
                for (int c = 0; c < NVP; c++)
                    if (c < nup) e[c] = fma(-f, cdp[(int64_t)(nxp + c) * cpitch + z], e[c]);
            } else {
                const int zc = z - nyp;
#pragma unroll
                for (int c = 0; c < P; c++)
                    if (c >= nxp && c < nx) m[c] = fma(f, cdc[(int64_t)(c - nxp) * ccpitch + zc], m[c]);
#pragma unroll
                for (int c = 0; c < NVP; c++)
                    if (c >= nup && c < nv) e[c] = fma(-f, cdc[(int64_t)(nxc + c - nup) * ccpitch + zc], e[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < NW; c++) {
            if (c < nw) {
                gw[c] = a.G[((int64_t)r + (int64_t)nv * c) * a.g_e + i * a.g_s];
                fin = fin && is_fin(gw[c]);
            }
        }
    }

    // ---- [I | M | Nw] by Gauss-Jordan elimination: fbg::gj_solve's loop with rhs = [m | gw], mirrored by hand (see the head of this file)
    bool used = !live, ok = true;
    int myk = 0;
#pragma unroll
    for (int k = 0; k < NVP; k++) {
        if (k < nv) {
            const fbg::Pivot pv = g.pivot(used, used ? -1.0 : fabs(e[k]), k);
            ok = ok && pv.found;
            panel_sync();
            if (r == pv.p) {
                const double ip = 1.0 / e[k];
#pragma unroll
                for (int j = k + 1; j < NVP; j++) { e[j] *= ip; prow[j] = e[j]; }
#pragma unroll
                for (int j = 0; j < P; j++) { m[j] *= ip; prow[NVP + j] = m[j]; }
#pragma unroll
                for (int j = 0; j < NW; j++) { gw[j] *= ip; prow[NVP + P + j] = gw[j]; }
                used = true; myk = k;
            }
            panel_sync();
            if (live && r != pv.p) {
                const double f = e[k];
#pragma unroll
                for (int j = k + 1; j < NVP; j++) e[j] = fma(-f, prow[j], e[j]);
                const double2* row = reinterpret_cast<const double2*>(prow + NVP);
#pragma unroll
                for (int j = 0; j < P; j += 2) {
                    const double2 s = row[j / 2];
                    m[j] = fma(-f, s.x, m[j]);
                    m[j + 1] = fma(-f, s.y, m[j + 1]);
                }
#pragma unroll
                for (int j = 0; j < NW; j += 2) {
                    const double2 s = row[(P + j) / 2];
                    gw[j] = fma(-f, s.x, gw[j]);
                    gw[j + 1] = fma(-f, s.y, gw[j + 1]);
                }
            }
        }
    }
    panel_sync();
    if (live) {
#pragma unroll
        for (int j = 0; j < P; j++) sol[myk * LD + j] = m[j];
#pragma unroll
        for (int j = 0; j < NW; j++) sol[myk * LD + P + j] = gw[j];
    }
    panel_sync();

    // ---- the system's status (the pivots' sizes are not kept: no rpiv is stored)
    const int32_t status = verdict<P>(g, fin, Solve{ok, 1.0, 1.0}, FB_CONNECT_NOT_FINITE, FB_CONNECT_ILL_POSED).status;
    const bool good = status == 0;
    const double nan = __builtin_nan("");
    if (valid && r == 0 && a.status) a.status[i] = status;

    // ---- row r of [A' | B']: the row's own block of B times [M | Nw]
    if (r < nx) {
        const bool inp = r < nxp;
        const int rc = r - nxp;
        double ar[P], br[NW];
#pragma unroll
        for (int c = 0; c < P; c++) {
            double v = 0.0;
            if (inp) { if (c < nxp) v = a.p.ab[ab_index(Sp, slotp, c) + r]; }
            else if (c >= nxp && c < nx) v = a.c.ab[ab_index(Sc, slotc, c - nxp) + rc];
            ar[c] = v;
        }
#pragma unroll
        for (int c = 0; c < NW; c++) br[c] = 0.0;
        const int k0 = inp ? 0 : nup, k1 = inp ? nup : nv;
        for (int k = k0; k < k1; k++) {
            const double b = inp ? a.p.ab[ab_index(Sp, slotp, a.p.G + k) + r] : a.c.ab[ab_index(Sc, slotc, a.c.G + k - nup) + rc];
            const double* s = sol + k * LD;
#pragma unroll
            for (int c = 0; c < P; c++) ar[c] = fma(b, s[c], ar[c]);
#pragma unroll
            for (int c = 0; c < NW; c++) br[c] = fma(b, s[P + c], br[c]);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < P; c++)
                if (c < nx) a.AB[staged_index(n, i, nx, r, c)] = good ? ar[c] : nan;
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nw) a.AB[staged_index(n, i, nx, r, nx + c)] = good ? br[c] : nan;
        }
    }

    // ---- rows r, r + P, ... of [C' | D']
    for (int j = r; j < ny; j += P) {
        const int z = a.iz[j];
        const bool inp = z < nyp;
        const int zc = z - nyp;
        double cr[P], dr[NW];
#pragma unroll
        for (int c = 0; c < P; c++) {
            double v = 0.0;
            if (inp) { if (c < nxp) v = cdp[(int64_t)c * cpitch + z]; }
            else if (c >= nxp && c < nx) v = cdc[(int64_t)(c - nxp) * ccpitch + zc];
            cr[c] = v;
        }
#pragma unroll
        for (int c = 0; c < NW; c++) dr[c] = 0.0;
        const int k0 = inp ? 0 : nup, k1 = inp ? nup : nv;
        for (int k = k0; k < k1; k++) {
            const double d = inp ? cdp[(int64_t)(nxp + k) * cpitch + z] : cdc[(int64_t)(nxc + k - nup) * ccpitch + zc];
            const double* s = sol + k * LD;
#pragma unroll
            for (int c = 0; c < P; c++) cr[c] = fma(d, s[c], cr[c]);
#pragma unroll
            for (int c = 0; c < NW; c++) dr[c] = fma(d, s[P + c], dr[c]);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < P; c++)
                if (c < nx) a.CD[staged_index(n, i, ny, j, c)] = good ? cr[c] : nan;
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nw) a.CD[staged_index(n, i, ny, j, nx + c)] = good ? dr[c] : nan;
        }
    }
}

}  // namespace fbc
