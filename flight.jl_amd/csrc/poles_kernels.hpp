// poles_kernels.hpp — the poles of a batch of LinearizedSS models on the device (include/flightbatch.h: fb_lss_poles; host side:
// fb_poles.inc; docs/design/linearize.md, "Poles on the device"; numpy restatement, operation for operation: tests/poles_prototype.py).
//   input check -> Parlett-Reinsch balancing by powers of two (no permutation) -> Householder reduction to Hessenberg form ->
//   Francis double-shift QR with deflation (EISPACK's balanc / orthes / hqr, eigenvalues only) -> dampreport's order.
// One system per group of P lanes of one wave (P = 8, 16 or 32, the smallest with P >= nx; 64 / P systems per wave, one wave per workgroup).
// The indices of this algorithm are data (the window [l, nn], the reflector's start m), so the matrix lives in the group's LDS panel, P rows
// at a pitch of P + 1 doubles (a lane per row or a lane per column, neither collides on a bank); column P of the panel, the padding, holds the
// Householder vector. A lane keeps scalars only; the scalars of a step are computed redundantly by every lane of the group from broadcast
// reads. The panel belongs to one wave: fences and wave_barrier (panel_sync), no s_barrier.
// The groups of a wave need not agree on anything: every loop runs over the range the wave's groups need together and a group takes part in a
// step by predicate; cross-lane operations (butterflies, ballots) stand outside the predicated regions. Every loop is bounded by a constant
// or by nx: a group that is finished, or whose input was not finite (its panel is zeroed: it deflates nx zero roots without a sweep), keeps
// its results until the wave's last group is done. Lanes past the batch's end redo the last system and store nothing.
#pragma once
#include "lss_group.hpp"
#include "../../include/flightbatch.h"

namespace fbe {

using namespace fbg;

constexpr int POLES_WAVE = fbg::WAVE;
constexpr int POLES_BAL_SWEEPS = 16, POLES_WINDOW_SWEEPS = 30, POLES_BAL_KMAX = 500;

struct PolesArgs {
    const double* ab;      // the handle's [A | B] (fbg::ab_index, lss_group.hpp), with its group size G
    double *re, *im;       // [nx x n], sorted; either may be null
    int32_t *iters, *status;
    int64_t n;
    int nx, G;
};

template <int P>
__global__ __launch_bounds__(POLES_WAVE) void k_poles(PolesArgs a) {
    constexpr int LD = P + 1, PANEL = P * LD, NG = POLES_WAVE / P;
    __shared__ double lds[NG * PANEL];
    const fbg::Lanes<P> g;
    double* const pan = lds + (threadIdx.x / P) * PANEL;
    const int r = g.r, nx = a.nx;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < a.n;
    const int64_t i = valid ? i_own : a.n - 1;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const bool act = r < nx;
    auto at = [&](int row, int col) -> double& { return pan[row * LD + col]; };

    // ---- the matrix into the panel (rows and columns past nx: zeros); a non-finite entry zeroes the group's panel
    bool fin = true;
    for (int c = 0; c < P; c++) {
        const double v = (act && c < nx) ? a.ab[ab_index(S, slot0, c) + r] : 0.0;
        fin = fin && is_fin(v);
        at(r, c) = v;
    }
    at(r, P) = 0.0;
    int status = g.any(!fin) ? FB_POLES_NOT_FINITE : 0;
    panel_sync();
    if (status) {
        for (int c = 0; c < P; c++) at(r, c) = 0.0;
    }
    panel_sync();

    // ---- balancing: row i / f, column i * f with f = 2^k, i in turn
#pragma unroll 1
    for (int sweep = 0; sweep < POLES_BAL_SWEEPS; sweep++) {
        bool changed = false;
#pragma unroll 1
        for (int bi = 0; bi < nx; bi++) {
            const bool off = act && r != bi;
            const double aji = at(r, bi), aij = at(bi, r);
            const double c = gsum<P>(off ? fabs(aji) : 0.0), rs = gsum<P>(off ? fabs(aij) : 0.0);
            bool take = false;
            double f = 1.0, fi = 1.0;
            if (c > 0.0 && rs > 0.0 && is_fin(c) && is_fin(rs)) {
                int ec, er;
                (void)frexp(c, &ec);
                (void)frexp(rs, &er);
                int k = min(max((er - ec) >> 1, -POLES_BAL_KMAX), POLES_BAL_KMAX);
                double c2 = ldexp(c, 2 * k);
                if (c2 < 0.5 * rs && k < POLES_BAL_KMAX) { k += 1; c2 = 4.0 * c2; }
                f = ldexp(1.0, k); fi = ldexp(1.0, -k);
                take = (c2 + rs) * fi < 0.95 * (c + rs);
            }
            panel_sync();
            if (take && off) { at(bi, r) = aij * fi; at(r, bi) = aji * f; }
            changed = changed || take;
            panel_sync();
        }
        if (__ballot(changed) == 0) break;
    }

    // ---- Hessenberg form: step m reflects column m - 1 below the subdiagonal
#pragma unroll 1
    for (int m = 1; m < nx - 1; m++) {
        const bool low = act && r >= m;
        const double col = low ? at(r, m - 1) : 0.0;
        const double scale = gsum<P>(fabs(col));
        const bool go = scale > 0.0;
        double o = go ? col / scale : 0.0;
        double h = gsum<P>(o * o);
        const double om = __shfl(o, m, P);
        const double gg = -copysign(sqrt(h), om);
        h = h - om * gg;
        if (r == m) o = o - gg;
        panel_sync();
        at(r, P) = o;
        panel_sync();
        if (go && low) {             // lane j = r, columns m ... nx - 1: v' A[:, j]
            double f = 0.0;
            for (int q = m; q < nx; q++) f = f + at(q, P) * at(q, r);
            f = f / h;
            for (int q = m; q < nx; q++) at(q, r) = at(q, r) - f * at(q, P);
        }
        panel_sync();
        if (go && act) {             // lane i = r, every row: A[i, :] v
            double f = 0.0;
            for (int q = m; q < nx; q++) f = f + at(q, P) * at(r, q);
            f = f / h;
            for (int q = m; q < nx; q++) at(r, q) = at(r, q) - f * at(q, P);
        }
        panel_sync();
        if (go && low) at(r, m - 1) = r == m ? scale * gg : 0.0;
        panel_sync();
    }

    // ---- the norm of the Hessenberg part (the small-subdiagonal test's scale where both diagonal neighbours are zero)
    double anorm;
    {
        double cs = 0.0;
        for (int q = 0; q < nx; q++) cs = cs + ((act && r >= q - 1) ? fabs(at(q, r)) : 0.0);
        anorm = gsum<P>(cs);
    }

    // ---- QR iteration on the window [l, nn], deflating from the bottom
    double wr = 0.0, wi = 0.0, t = 0.0;
    int nn = nx - 1, its = 0, iters = 0;
    const int bound = (POLES_WINDOW_SWEEPS + 1) * nx + 1;
#pragma unroll 1
    for (int step = 0; step < bound; step++) {
        const bool run = nn >= 0;
        if (__ballot(run) == 0) break;
        const int en = run ? nn : 0;           // (a finished group reads its corner and takes no part)
        // the lowest-right small subdiagonal element: lane r tests a[r][r - 1]
        int l;
        {
            const int rc = act ? r : 0, rm = rc > 0 ? rc - 1 : 0;
            double s = fabs(at(rm, rm)) + fabs(at(rc, rc));
            if (s == 0.0) s = anorm;
            const bool small = fabs(at(rc, rm)) + s == s;
            const unsigned msk = g.mask(run && small && r >= 1 && r <= en && act);
            l = msk ? 31 - __builtin_clz(msk) : 0;
        }
        panel_sync();
        if (run && l > 0 && r == 0) at(l, l - 1) = 0.0;
        panel_sync();
        const int e1 = en > 0 ? en - 1 : 0, e2 = en > 1 ? en - 2 : 0;
        double x = at(en, en), y = at(e1, e1), w = at(en, e1) * at(e1, en);
        bool sw = false;
        if (run) {
            if (l == en) {
                if (r == en) { wr = x + t; wi = 0.0; }
                nn -= 1; its = 0;
            } else if (l == en - 1) {
                const double p = 0.5 * (y - x), q = p * p + w;
                double z = sqrt(fabs(q));
                const double xt = x + t;
                double r0, r1, i0, i1;   // roots at en - 1 and en
                if (q >= 0.0) {
                    z = p + copysign(z, p);
                    r0 = xt + z;
                    r1 = z != 0.0 ? xt - w / z : r0;
                    i0 = i1 = 0.0;
                } else {
                    r0 = r1 = xt + p;    // a pair: the same Re bits, +-Im
                    i0 = z; i1 = -z;
                }
                if (r == en - 1) { wr = r0; wi = i0; }
                if (r == en) { wr = r1; wi = i1; }
                nn -= 2; its = 0;
            } else if (its == POLES_WINDOW_SWEEPS) {
                status |= FB_POLES_NOT_CONVERGED;
                nn = -1;
            } else {
                sw = true;
            }
        }
        if (__ballot(sw) == 0) continue;

        // ---- one double-shift sweep for the groups with sw
        const bool exc = sw && (its == 10 || its == 20);
        panel_sync();
        if (exc && r <= en) at(r, r) = at(r, r) - x;
        panel_sync();
        if (exc) {
            t = t + x;
            const double s = fabs(at(en, e1)) + fabs(at(e1, e2));
            x = y = 0.75 * s;
            w = -0.4375 * s * s;
        }
        if (sw) { its++; iters++; }
        // the reflector's start m: the highest m in [l, en - 2] that is l or passes the two-small-subdiagonals test; lane r tests m = r
        int m;
        double p, q, rr;
        auto start = [&](int mm, double& p_, double& q_, double& r_) {
            const double z = at(mm, mm);
            double r0 = x - z, s = y - z;
            p_ = (r0 * s - w) / at(mm + 1, mm) + at(mm, mm + 1);
            q_ = at(mm + 1, mm + 1) - z - r0 - s;
            r_ = at(mm + 2, mm + 1);
            s = fabs(p_) + fabs(q_) + fabs(r_);
            p_ = p_ / s; q_ = q_ / s; r_ = r_ / s;
        };
        {
            const bool cand = sw && r >= l && r <= en - 2;
            const int mm = cand ? r : e2, mb = mm > 0 ? mm - 1 : 0;     // (e2 + 2 <= en whenever sw; otherwise rows 0 ... 2 of the panel)
            start(mm, p, q, rr);
            const double u = fabs(at(mm, mb)) * (fabs(q) + fabs(rr));
            const double v = fabs(p) * (fabs(at(mb, mb)) + fabs(at(mm, mm)) + fabs(at(mm + 1, mm + 1)));
            const unsigned msk = g.mask(cand && (r == l || u + v == v));
            m = msk ? 31 - __builtin_clz(msk) : e2;
            start(m, p, q, rr);
        }
        const int kLo = wave_min<P>(sw ? m : P), kHi = wave_max<P>(sw ? en - 1 : -1);
#pragma unroll 1
        for (int k = kLo; k <= kHi; k++) {
            const bool in = sw && k >= m && k < en;
            const bool last = k == en - 1;
            bool go = in;
            panel_sync();
            if (in && k != m) {
                p = at(k, k - 1); q = at(k + 1, k - 1); rr = last ? 0.0 : at(k + 2, k - 1);
                x = fabs(p) + fabs(q) + fabs(rr);
                go = x != 0.0;
                if (go) { p = p / x; q = q / x; rr = rr / x; }
            }
            panel_sync();
            if (go) {
                const double s = copysign(sqrt(p * p + q * q + rr * rr), p);
                if (r == 0) {
                    if (k == m) {
                        if (l != m) at(k, k - 1) = -at(k, k - 1);
                    } else {
                        at(k, k - 1) = -s * x;
                        at(k + 1, k - 1) = 0.0;
                        if (!last) at(k + 2, k - 1) = 0.0;
                    }
                }
                p = p + s;
                x = p / s; y = q / s;
                const double z = rr / s;
                q = q / p; rr = rr / p;
                if (r >= k && r <= en) {                 // lane j = r of columns k ... en: rows k, k + 1, k + 2
                    double pp = at(k, r) + q * at(k + 1, r);
                    if (!last) {
                        pp = pp + rr * at(k + 2, r);
                        at(k + 2, r) = at(k + 2, r) - pp * z;
                    }
                    at(k + 1, r) = at(k + 1, r) - pp * y;
                    at(k, r) = at(k, r) - pp * x;
                }
                panel_sync();
                if (r >= l && r <= min(en, k + 3)) {     // lane i = r of rows l ... min(en, k + 3): columns k, k + 1, k + 2
                    double pp = x * at(r, k) + y * at(r, k + 1);
                    if (!last) {
                        pp = pp + z * at(r, k + 2);
                        at(r, k + 2) = at(r, k + 2) - pp * rr;
                    }
                    at(r, k + 1) = at(r, k + 1) - pp * q;
                    at(r, k) = at(r, k) - pp;
                }
            }
        }
        panel_sync();
    }
    if (nn >= 0) status |= FB_POLES_NOT_CONVERGED;     // (the step bound: unreachable, every step deflates or sweeps)
    if (status == 0 && g.any(act && !(is_fin(wr) && is_fin(wi)))) status = FB_POLES_NOT_FINITE;

    // ---- the order: |pole|, Re, Im, position; every lane counts the poles that precede its own
    const double wn = sqrt(wr * wr + wi * wi);
    panel_sync();
    at(0, r) = wn; at(1, r) = wr; at(2, r) = wi;
    panel_sync();
    int rank = 0;
    for (int j = 0; j < nx; j++) {
        const double nj = at(0, j), rj = at(1, j), ij = at(2, j);
        const bool before = nj < wn || (nj == wn && (rj < wr || (rj == wr && (ij < wi || (ij == wi && j < r)))));
        rank += (j != r && before) ? 1 : 0;
    }
    if (!valid) return;
    const double nan = __builtin_nan("");
    if (act) {
        // (a system with a status stores NaN in its own place: its ranks are meaningless)
        const int64_t row = status ? r : rank;
        if (a.re) a.re[row * a.n + i] = status ? nan : wr;
        if (a.im) a.im[row * a.n + i] = status ? nan : wi;
    }
    if (r == 0) {
        if (a.iters) a.iters[i] = iters;
        if (a.status) a.status[i] = status;
    }
}

}  // namespace fbe
