// margins_kernels.hpp — gain and phase margins of a batch of loops on the device (include/flightbatch.h: fb_lss_margins; host side:
// fb_margins.inc; docs/design/linearize.md, "Margins on the device"; numpy restatement: tests/margins_prototype.py). Reference:
// FA design/robot2d/robot2d_design.ipynb — `marginplot(P_v[:η, :v_ref])` and `marginplot(series(C_η2v, P_v2η))` with k_p_η2v = 0.6.
//   loop      L(jw) = gain (c inv(jw I - A) b + d) of channel (iu, iy) in deviation coordinates; negative unity feedback, 1 + L
//   stage 1   fbp::k_lss_freqresp (pid_kernels.hpp) has put c inv(jw I - A) b + d on the caller's grid into re, im [nw x n]: 2 nw n doubles
//             on the device for the length of the call, 5.1 GB at a million systems and the default 321 frequencies (fb_pid_metrics' footprint)
//   stage 2   k_lss_margins, here: one system per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx)
// The scan: lane r takes the intervals r, r + P, ... of its system's row of the grid, applies the gain, and the brackets of 64 intervals
// become two 64-bit words of group ballots (phase: the sign of Im L changes and Re L < 0 at an end; gain: |L|^2 - 1 changes sign), kept in
// the group's LDS; the smallest |1 + L|^2 of the grid is reduced over the group, the lower frequency at a tie.
// The refinement: a group pops its lowest pending bracket (the phase brackets first) and bisects it geometrically, mid = sqrt(lo hi), on the
// bracket's own predicate, at most MG_ITERS times, every evaluation of L(j mid) one complex Gauss-Jordan elimination by the whole group.
// The trip count is the wave's: the loop runs while any group of the wave has a bracket pending; a group that has finished evaluates its
// last frequency again and stores nothing. The crossing is the final lo with the L that was evaluated there. Selection is by comparisons
// of products, no division and no transcendental: gm, pm and smin = sqrt are the host's (fb_margins.inc).
// Lanes past the batch's end work on the last system and store nothing, so a wave never diverges on the batch size.
#pragma once
#include "freq_group.hpp"   // mag2, closer_to_one
#include "../../include/flightbatch.h"

namespace fbn {

using namespace fbg;

constexpr int MG_ITERS = 60;      // the cap of a bisection; from a 321-point grid it ends by itself after 47 or 48 halvings
constexpr int MG_CHUNKS = 16;     // 64-interval chunks of the largest grid (1024 frequencies)

struct MarginArgs {
    const double* ab; const double* cd;   // the handle's copies (fbg::ab_index, lss_group.hpp), G its group size
    const double* w;                      // [nw]
    const double* re; const double* im;   // c inv(jw I - A) b + d on the grid, [nw x n], NaN where stage 1 found no pivot
    const double* gain;                   // [n] or null (ones)
    double* sel;                          // [10 x n]: rows 1 and 3 .. 9 of fb_lss_margins' sel, row 8 as smin^2; rows 0 and 2 are the host's
    double* all;                          // [6 x FB_MARGINS_KMAX x n] or null: per kind (phase, gain) w*, Re L*, Im L*
    int32_t* counts;                      // [2 x n]
    int32_t* status;                      // [n]
    int64_t n;
    int nx, nu, ny, G, iu, iy, nw;
};

template <int P>
__global__ __launch_bounds__(WAVE) void k_lss_margins(MarginArgs a) {
    constexpr int NG = WAVE / P, PER = 64 / P, KMAX = FB_MARGINS_KMAX;
    constexpr int GD = 2 * (P + 1) + 2 * P + P + 2 * MG_CHUNKS;   // doubles per group: pivot row | solution | c | bracket words
    __shared__ __attribute__((aligned(16))) double lds[NG * GD];
    const Lanes<P> g;
    double2* pan = reinterpret_cast<double2*>(lds + (threadIdx.x / P) * GD);   // P + 1 complex numbers: the scaled pivot row, its right-hand side last
    double2* xs = pan + (P + 1);
    double* cv = reinterpret_cast<double*>(xs + P);
    unsigned long long* msk = reinterpret_cast<unsigned long long*>(cv + P);   // [2 x MG_CHUNKS]: phase, gain
    const int r = g.r, nx = a.nx, nw = a.nw;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t S = n * a.G, slot0 = i * a.G;
    const bool live = r < nx, store = valid && r == 0;
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    // ---- this lane's row of [-A | b], c into the panel, d and the gain; whether all of that is finite
    double na[P];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < P; c++) {
        na[c] = (live && c < nx) ? -a.ab[ab_index(S, slot0, c) + r] : 0.0;
        fin = fin && is_fin(na[c]);
    }
    const double b0 = live ? a.ab[ab_index(S, slot0, a.G + a.iu) + r] : 0.0;
    const double c0 = live ? a.cd[cd_index(n, i, a.ny, a.iy, r)] : 0.0;
    const double d = a.cd[cd_index(n, i, a.ny, a.iy, nx + a.iu)];
    const double gn = a.gain ? a.gain[i] : 1.0;
    const bool notfin = g.any(!(fin && is_fin(b0) && is_fin(c0) && is_fin(d) && is_fin(gn)));
    cv[r] = c0;

    // L(j om) / gain of this group's system; false where a pivot was zero or not finite, or the value is not finite. The elimination is
    // k_lss_freqresp's (pid_kernels.hpp), step for step, kept beside it so that kernel's code stays what it was: the family's pivot rule on
    // |z|^2, the scaled pivot row through the group's panel, every step a compile-time index
    auto response = [&](double om, double& pr, double& pi) -> bool {
        double zr[P], zi[P];
#pragma unroll
        for (int c = 0; c < P; c++) {
            zr[c] = na[c];
            zi[c] = c == r ? om : 0.0;
        }
        double br = b0, bi = 0.0;
        bool used = !live, ok = true;
        int myk = r;
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
        // the lane that was the pivot of step k holds x_k: d + sum_k c_k x_k, k ascending
        panel_sync();
        if (live) xs[myk] = make_double2(br, bi);
        panel_sync();
        pr = d; pi = 0.0;
        for (int k = 0; k < nx; k++) {
            const double ck = cv[k];
            const double2 x = xs[k];
            pr = fma(ck, x.x, pr);
            pi = fma(ck, x.y, pi);
        }
        return ok && is_fin(pr) && is_fin(pi);
    };

    // ---- the scan: brackets of 64 intervals per pass as group ballots, the grid's smallest |1 + L|^2
    const int nch = (nw - 1 + 63) / 64;
    double s2 = inf;
    int ks = INT32_MAX;
    bool bad = false;
    unsigned sump = 0, sumg = 0;   // the chunks with a pending phase / gain bracket
    for (int c = 0; c < nch; c++) {
        unsigned long long mp = 0, mg = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int k = 64 * c + P * j + r;
            bool bp = false, bg = false;
            if (k + 1 < nw) {
                const double l0r = gn * a.re[(int64_t)k * n + i], l0i = gn * a.im[(int64_t)k * n + i];
                const double l1r = gn * a.re[(int64_t)(k + 1) * n + i], l1i = gn * a.im[(int64_t)(k + 1) * n + i];
                bad = bad || !is_fin(l0r) || !is_fin(l0i) || !is_fin(l1r) || !is_fin(l1i);
                const double v0 = mag2(1.0 + l0r, l0i), v1 = mag2(1.0 + l1r, l1i);
                if (v0 < s2) { s2 = v0; ks = k; }
                if (k + 2 == nw && v1 < s2) { s2 = v1; ks = k + 1; }   // the grid's last point has no interval of its own
                bp = ((l0i < 0.0) != (l1i < 0.0)) && !(l0r >= 0.0 && l1r >= 0.0);   // (both ends right of the axis: the positive real axis)
                bg = (mag2(l0r, l0i) < 1.0) != (mag2(l1r, l1i) < 1.0);
            }
            mp |= (unsigned long long)g.mask(bp) << (P * j);
            mg |= (unsigned long long)g.mask(bg) << (P * j);
        }
        if (r == 0) { msk[c] = mp; msk[MG_CHUNKS + c] = mg; }
        sump |= (unsigned)(mp != 0) << c;
        sumg |= (unsigned)(mg != 0) << c;
    }
    const double s2g = -g.gmax(-s2);
    int ksg = s2 == s2g ? ks : INT32_MAX;
#pragma unroll
    for (int o = P / 2; o > 0; o >>= 1) ksg = min(ksg, __shfl_xor(ksg, o, P));
    bool sing = g.any(bad);
    if (notfin || sing) sump = sumg = 0;
    panel_sync();

    // ---- the refinement. Everything below is uniform within a group.
    unsigned long long curp = 0, curg = 0;   // what is left of the chunk a kind is in, and that chunk's first interval
    int basep = 0, baseg = 0;
    bool active = false, plo = false, trunc = false;
    int kind = 0, it = 0, npc = 0, ngc = 0;
    double lo = a.w[0], hi = lo, llr = 0.0, lli = 0.0;             // the bracket and L at lo
    double wpc = nan, pcr = nan, pci = nan, wgc = nan, gcr = nan, gci = nan, gnum = 0.0, gden = 1.0;
    auto pending = [&] { return (curp | curg) != 0 || (sump | sumg) != 0; };
    auto before = [&](double lr, double li) { return kind == 0 ? li < 0.0 : mag2(lr, li) < 1.0; };   // the bracket's predicate
    auto pop = [&] {
        kind = (curp != 0 || sump != 0) ? 0 : 1;
        unsigned long long cur = kind == 0 ? curp : curg;
        unsigned sum = kind == 0 ? sump : sumg;
        int cb = kind == 0 ? basep : baseg;
        if (cur == 0) {
            const int c = __builtin_ctz(sum);
            cur = msk[kind * MG_CHUNKS + c];
            sum &= sum - 1;
            cb = 64 * c;
        }
        const int k = cb + __builtin_ctzll(cur);
        cur &= cur - 1;
        if (kind == 0) { curp = cur; sump = sum; basep = cb; } else { curg = cur; sumg = sum; baseg = cb; }
        if (kind == 1 && ngc == KMAX) { trunc = true; curg = 0; sumg = 0; return; }   // (a gain bracket always counts: nothing to refine)
        lo = a.w[k]; hi = a.w[k + 1];
        llr = gn * a.re[(int64_t)k * n + i]; lli = gn * a.im[(int64_t)k * n + i];
        plo = before(llr, lli);
        it = 0; active = true;
    };
    auto record = [&] {
        if (kind == 0) {
            if (!(llr < 0.0)) return;
            if (npc == KMAX) { trunc = true; curp = 0; sump = 0; return; }
            if (npc == 0 || closer_to_one(-llr, -pcr)) { wpc = lo; pcr = llr; pci = lli; }
        } else {
            // the largest -Re L* / |L*|, as sign(x) x^2 / |L*|^2 by cross-multiplication
            const double num = -llr * fabs(llr), den = mag2(llr, lli);
            const double ours = num * gden, theirs = gnum * den;
            if (ngc == 0 || ours > theirs) { wgc = lo; gcr = llr; gci = lli; gnum = num; gden = den; }
        }
        const int slot = kind == 0 ? npc : ngc;
        if (a.all && store) {
            double* q = a.all + ((int64_t)(3 * kind) * KMAX + slot) * n + i;
            q[0] = lo; q[(int64_t)KMAX * n] = llr; q[2 * (int64_t)KMAX * n] = lli;
        }
        if (kind == 0) npc++; else ngc++;
    };
    for (;;) {
        // a bracket that has ended is recorded and the next one popped in the same trip
        bool step = false;
        double om = lo;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (!step) {
                if (!active && pending()) pop();
                if (active) {
                    const double mid = sqrt(lo * hi);
                    if (mid > lo && mid < hi && it < MG_ITERS) { step = true; om = mid; }
                    else { record(); active = false; }
                }
            }
        }
        if (!__any(active || pending())) break;
        double lr, li;
        const bool ok = response(om, lr, li);
        if (step) {
            lr *= gn; li *= gn;
            if (!ok) { sing = true; active = false; curp = curg = 0; sump = sumg = 0; }
            else {
                it++;
                if (before(lr, li) == plo) { lo = om; llr = lr; lli = li; } else hi = om;
            }
        }
    }

    // ---- what the system leaves: a status that voids it stores NaN and zero counts
    const bool voided = notfin || sing;
    if (a.all && valid) {
        for (int e = r; e < 6 * KMAX; e += P) {
            const int slot = e % KMAX, knd = e / (3 * KMAX);
            if (voided || slot >= (knd == 0 ? npc : ngc)) a.all[(int64_t)e * n + i] = nan;
        }
    }
    if (!store) return;
    const double out[10] = {nan, wpc, nan, wgc, pcr, pci, gcr, gci, s2g, ksg < nw ? a.w[ksg] : nan};
#pragma unroll
    for (int k = 0; k < 10; k++) a.sel[(int64_t)k * n + i] = voided ? nan : out[k];
    a.counts[i] = voided ? 0 : npc;
    a.counts[n + i] = voided ? 0 : ngc;
    a.status[i] = notfin ? FB_MARGINS_NOT_FINITE : sing ? FB_MARGINS_SINGULAR : trunc ? FB_MARGINS_TRUNCATED : 0;
}

}  // namespace fbn
