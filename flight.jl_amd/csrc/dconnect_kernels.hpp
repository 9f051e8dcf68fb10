// dconnect_kernels.hpp — connect for a batch of SAMPLED linear models with unit delays on the device (include/flightbatch.h: fb_lss_dconnect;
// host side: fb_dconnect.inc; docs/design/linearize.md, "Closing sampled loops on the device"; numpy restatement: tests/dconnect_prototype.py).
//   plant p and compensator c as in connect_kernels.hpp, both sampled: x+ = A x + B v, z = C x + D v with x = [x_p; x_c], v = [u_p; u_c],
//   z = [y_p; y_c] (nz rows), block-diagonal. dz [nd] names rows of z that are also kept one sample: q_k(t) = z[dz_k](t - 1). The extended
//   model has the states xe = [x; q] (nxe = nx + nd) and the signals ze = [z; q]:
//       Ae = [[A, 0], [C[dz], 0]],  Be = [B; D[dz]],  Ce = [[C, 0], [0, I]],  De = [D; 0]
//   Interconnection v = F ze[jz] + G w, outputs ze[iz]: k_connect's formula on the extended model,
//       E = inv(I - F De[jz, :]), M = E F Ce[jz, :], Nw = E G;  A' = Ae + Be M, B' = Be Nw, C' = Ce[iz, :] + De[iz, :] M, D' = De[iz, :] Nw.
// The shape is k_connect's: one system per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= max(nxe, nv)), lane r < nv owns
// row r of [I - F D_jz | F Ce_jz | G] (the middle block has nxe columns), the same Gauss-Jordan elimination written out, [M | Nw] through the
// group's LDS panel, fences and wave_barrier, lanes past the batch's end redo the last system and store nothing. The zero and unit blocks
// of the extended model are skipped:
//   a read jz >= nz adds its F entry to column nx + (jz - nz) of the middle block and reads nothing from either model;
//   state lane r < nx forms row r of [A | 0] + B_r [M | Nw] (M's delay columns land in a row that is zero there);
//   state lane r in [nx, nxe) forms the delay row [C[dz_k] | 0] + D[dz_k] [M | Nw], k = r - nx: an output row of k_connect, stored in [A' | B'];
//   an output row iz >= nz is a unit row: stored, not multiplied.
// Every sum runs with k ascending as explicit fma, in k_connect's order: with nd = 0 the result has the bits k_connect gives on the same four
// matrices. The result goes to a staging block in fb_linearize's layout; fbl::k_lss_gather makes the new handle's copy from it.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbv {

using namespace fbg;

constexpr int DC_WAVE = fbg::WAVE;
constexpr int DC_NW_MAX = 8;      // the inputs of the new model: fbl::LSS_NU_MAX

struct DConnectSide {
    const double* ab; const double* cd;   // a handle's copies (fbg::ab_index, lss_group.hpp), G its group size
    int nx, nu, ny, G;
};
struct DConnectArgs {
    DConnectSide p, c;                    // c: all sizes 0 when there is no compensator
    const int32_t* jz; const int32_t* iz; // [nf], [ny]: rows of ze = [z; q]
    const int32_t* dz;                    // [nd]: rows of z
    const double* F; const double* G;     // element (r, k) at [(r + nv k) fe + i fs]: (fe, fs) = (1, 0) for the batch's matrix, (n, 1) per system
    int64_t f_e, f_s, g_e, g_s;
    double* AB; double* CD;               // staging, fb_linearize's layout: [(r + nxe c) n + i] over nxe + nw columns, [(j + ny c) n + i]
    int32_t* status;
    int64_t n;
    int nf, nw, ny, nd;
};

template <int P>
__global__ __launch_bounds__(DC_WAVE) void k_dconnect(DConnectArgs a) {
    constexpr int NVP = P < FB_CONNECT_NV_MAX ? P : FB_CONNECT_NV_MAX, NW = DC_NW_MAX;
    constexpr int ROW = NVP + P + NW, LD = P + NW + 1, NG = DC_WAVE / P, GRP = ROW + NVP * LD;   // (ROW and GRP are even: 16-byte rows)
    __shared__ __attribute__((aligned(16))) double lds[NG * GRP];
    const fbg::Lanes<P> g;
    double* prow = lds + (threadIdx.x / P) * GRP;   // the scaled pivot row of the current step: e | m | gw
    double* sol = prow + ROW;                       // [M | Nw], NVP x LD
    const int r = g.r;
    const int nxp = a.p.nx, nup = a.p.nu, nyp = a.p.ny, nxc = a.c.nx, nuc = a.c.nu;
    const int nx = nxp + nxc, nv = nup + nuc, nz = nyp + a.c.ny, nf = a.nf, nw = a.nw, ny = a.ny;
    const int nxe = nx + a.nd;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t Sp = n * a.p.G, slotp = i * a.p.G, Sc = n * a.c.G, slotc = i * a.c.G;
    // cd_index at unrolled columns, base and column pitch hoisted by hand, as in k_connect: (z, col) at cdp[col cpitch + z]
    const double* cdp = a.p.cd + i * nyp;
    const double* cdc = a.c.cd + i * a.c.ny;
    const int64_t cpitch = n * nyp, ccpitch = n * a.c.ny;

    // ---- every entry of the sources
    bool fin = model_finite<P>(a.p.ab, a.p.cd, nxp, nup, nyp, a.p.G, n, i, r);
    if (nxc > 0) fin = fin && model_finite<P>(a.c.ab, a.c.cd, nxc, nuc, a.c.ny, a.c.G, n, i, r);

    // ---- this lane's row of [I - F D_jz | F Ce_jz | G]
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
            } else if (z < nz) {
                const int zc = z - nyp;
#pragma unroll
                for (int c = 0; c < P; c++)
                    if (c >= nxp && c < nx) m[c] = fma(f, cdc[(int64_t)(c - nxp) * ccpitch + zc], m[c]);
#pragma unroll
                for (int c = 0; c < NVP; c++)
                    if (c >= nup && c < nv) e[c] = fma(-f, cdc[(int64_t)(nxc + c - nup) * ccpitch + zc], e[c]);
            } else {
                const int cq = nx + (z - nz);   // a delayed read: a unit row of Ce, a zero row of De
#pragma unroll
                for (int c = 0; c < P; c++)
                    if (c == cq) m[c] = m[c] + f;
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

    // ---- [I | M | Nw] by Gauss-Jordan elimination: k_connect's loop (fbg::gj_solve with rhs = [m | gw], mirrored by hand)
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

    // ---- row r of [A' | B']: r < nx, the row's own block of B times [M | Nw]; r >= nx, the delay row: row dz[r - nx] of [C | D] likewise
    if (r < nxe) {
        const bool state = r < nx;
        const int z = state ? 0 : a.dz[r - nx];
        const bool inp = state ? r < nxp : z < nyp;
        const int rc = r - nxp, zc = z - nyp;
        double ar[P], br[NW];
#pragma unroll
        for (int c = 0; c < P; c++) {
            double v = 0.0;
            if (inp) { if (c < nxp) v = state ? a.p.ab[ab_index(Sp, slotp, c) + r] : cdp[(int64_t)c * cpitch + z]; }
            else if (c >= nxp && c < nx) v = state ? a.c.ab[ab_index(Sc, slotc, c - nxp) + rc] : cdc[(int64_t)(c - nxp) * ccpitch + zc];
            ar[c] = v;
        }
#pragma unroll
        for (int c = 0; c < NW; c++) br[c] = 0.0;
        const int k0 = inp ? 0 : nup, k1 = inp ? nup : nv;
        for (int k = k0; k < k1; k++) {
            double b;
            if (state) b = inp ? a.p.ab[ab_index(Sp, slotp, a.p.G + k) + r] : a.c.ab[ab_index(Sc, slotc, a.c.G + k - nup) + rc];
            else b = inp ? cdp[(int64_t)(nxp + k) * cpitch + z] : cdc[(int64_t)(nxc + k - nup) * ccpitch + zc];
            const double* s = sol + k * LD;
#pragma unroll
            for (int c = 0; c < P; c++) ar[c] = fma(b, s[c], ar[c]);
#pragma unroll
            for (int c = 0; c < NW; c++) br[c] = fma(b, s[P + c], br[c]);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < P; c++)
                if (c < nxe) a.AB[staged_index(n, i, nxe, r, c)] = good ? ar[c] : nan;
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nw) a.AB[staged_index(n, i, nxe, r, nxe + c)] = good ? br[c] : nan;
        }
    }

    // ---- rows r, r + P, ... of [C' | D']: a row of z as in k_connect, a row of q a unit row
    for (int j = r; j < ny; j += P) {
        const int z = a.iz[j];
        const bool unit = z >= nz;
        const bool inp = z < nyp;
        const int zc = z - nyp, cq = nx + (z - nz);
        double cr[P], dr[NW];
#pragma unroll
        for (int c = 0; c < P; c++) {
            double v = 0.0;
            if (unit) { if (c == cq) v = 1.0; }
            else if (inp) { if (c < nxp) v = cdp[(int64_t)c * cpitch + z]; }
            else if (c >= nxp && c < nx) v = cdc[(int64_t)(c - nxp) * ccpitch + zc];
            cr[c] = v;
        }
#pragma unroll
        for (int c = 0; c < NW; c++) dr[c] = 0.0;
        const int k0 = inp ? 0 : nup, k1 = unit ? nup : inp ? nup : nv;   // (a unit row: no term)
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
                if (c < nxe) a.CD[staged_index(n, i, ny, j, c)] = good ? cr[c] : nan;
#pragma unroll
            for (int c = 0; c < NW; c++)
                if (c < nw) a.CD[staged_index(n, i, ny, j, nxe + c)] = good ? dr[c] : nan;
        }
    }
}

}  // namespace fbv
