// dfreq_kernels.hpp — frequency response and margins of a batch of SAMPLED loops on the device (include/flightbatch.h: fb_lss_dfreqresp,
// fb_lss_dmargins; host side: fb_dfreq.inc; docs/design/linearize.md, "Sampled loops on the device"; numpy restatement:
// tests/dmargins_prototype.py). Reference: the controllers of FP/control.jl run in f_periodic! at dt = 0.02 on gains designed in continuous
// time; ControlSystems' margin and freqresp on a discrete system evaluate it on the unit circle.
//   loop      L(z) = gain (c inv(z I - Phi) gamma + d) of channel (iu, iy) of a sampled handle, z = e^(j w Ts); negative unity feedback, 1 + L
//   the grid  arrives as cos(w_k Ts), sin(w_k Ts), formed by the host with the C library: no trigonometric function is evaluated here (the
//             device library is built with -fapprox-func). A frequency IS its point on the circle from here on.
//   k_lss_dfreqresp   one (system, frequency) pair per group of P lanes of one wave (P = 8, 16 or 32, the smallest >= nx), the shape of
//                     fbp::k_lss_freqresp (pid_kernels.hpp); it is also stage 1 of fb_lss_dmargins
//   k_lss_dmargins    one system per group, the shape of fbn::k_lss_margins (margins_kernels.hpp): the scan, the ballot words per 64-interval
//                     chunk, the predicates, pop / record and the wave-uniform trip count are that kernel's
// The elimination is written once, circle_response below: lane r owns the complex row r of [z I - Phi | gamma]. Its only arithmetic
// difference from the continuous kernels' is the diagonal: -Phi_rr + cos in the real part, sin in the imaginary part. The two continuous
// copies stay where they are, untouched (their instruction text is pinned).
// The refinement bisects the ARC, not the frequency: a bracket is a pair of points z_lo, z_hi of the circle, its midpoint
// (z_lo + z_hi) / |z_lo + z_hi|, one square root and one division, each component held between the ends' where it is monotone along the
// arc (rounding would otherwise leave it an ulp outside two neighbouring points for good). It ends when the midpoint equals an end in both
// components, or at the cap DM_ITERS. The crossing is the final z_lo with the L that was evaluated there; w* = atan2(Im z*, Re z*) / Ts is the host's, beside gm,
// pm and smin = sqrt (fb_dfreq.inc).
// Lanes past the batch's end work on the last system (pair) and store nothing, so a wave never diverges on the batch size.
#pragma once
#include "freq_group.hpp"   // mag2, closer_to_one
#include "../../include/flightbatch.h"

namespace fbw {

using namespace fbg;

// The cap of a bisection. tests/test_dmargins_host.py runs the numpy restatement over every test case and prints the largest halving
// count it sees: 53 (33- to 257-point grids; a bracket ends by itself after 47 to 53 halvings, when the arc has reached the rounding level
// of z). The cap is that figure plus 10, the relation of fbn::MG_ITERS = 60 to its observed 47 to 48. It is what ends a bracket that
// straddles pi / 2 to the last ulp, where the sine is not monotone and is left unclamped (below).
constexpr int DM_ITERS = 63;
constexpr int DM_CHUNKS = 16;     // 64-interval chunks of the largest grid (1024 frequencies)

// doubles of LDS per group: the scaled pivot row with its right-hand side (P + 1 complex) | the solution (P complex) | c
template <int P> constexpr int PANEL = 2 * (P + 1) + 2 * P + P;

struct DFreqArgs {
    const double* ab; const double* cd;   // the handle's copies (fbg::ab_index, lss_group.hpp), G its group size: Phi | Gamma, C | D
    const double* cs; const double* sn;   // [nw]: cos(w_k Ts), sin(w_k Ts)
    double *re, *im;                      // [nw x n], system index fastest; NaN where a pivot was zero or not finite
    int64_t n;
    int nx, nu, ny, G, iu, iy, nw;
};

struct DMarginArgs {
    const double* ab; const double* cd;
    const double* cs; const double* sn;   // [nw]
    const double* re; const double* im;   // c inv(z_k I - Phi) gamma + d on the grid, [nw x n], NaN where stage 1 found no pivot
    const double* gain;                   // [n] or null (ones)
    double* sel;                          // [10 x n]: Im z, Re z at the phase crossing | Im z, Re z at the gain crossing | Re L*, Im L* of each |
                                          // smin^2 | the grid index of smin as a double. The host turns rows 0 .. 3, 8 and 9 into the ABI's.
    double* all;                          // [8 x FB_MARGINS_KMAX x n] or null: per kind (phase, gain) Re z*, Im z*, Re L*, Im L*
    int32_t* counts;                      // [2 x n]
    int32_t* status;                      // [n]
    int64_t n;
    int nx, nu, ny, G, iu, iy, nw;
};

// c inv(z I - Phi) gamma + d at z = (cz, sz) for the system whose row r of [-Phi | gamma] this lane holds (np, g0), c in the group's cv, by
// the whole group: Gauss-Jordan with the family's pivot rule on |z|^2, the scaled pivot row through the group's panel, every step a
// compile-time index. False where a pivot was zero or not finite, or the value is not finite.
template <int P>
__device__ __forceinline__ bool circle_response(const Lanes<P>& g, const double (&np)[P], double g0, double d, int nx, bool live, double2* pan,
                                                double2* xs, const double* cv, double cz, double sz, double& pr, double& pi) {
    const int r = g.r;
    double zr[P], zi[P];
#pragma unroll
    for (int c = 0; c < P; c++) {
        zr[c] = c == r ? np[c] + cz : np[c];
        zi[c] = c == r ? sz : 0.0;
    }
    double br = g0, bi = 0.0;
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
}

template <int P>
__global__ __launch_bounds__(WAVE) void k_lss_dfreqresp(DFreqArgs a) {
    constexpr int NG = WAVE / P, GD = PANEL<P>;
    __shared__ __attribute__((aligned(16))) double lds[NG * GD];
    const Lanes<P> g;
    double2* pan = reinterpret_cast<double2*>(lds + (threadIdx.x / P) * GD);
    double2* xs = pan + (P + 1);
    double* cv = reinterpret_cast<double*>(xs + P);
    const int r = g.r, nx = a.nx;
    const int64_t total = a.n * a.nw;
    const int64_t q_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = q_own < total;
    const int64_t q = valid ? q_own : total - 1;
    const int64_t i = q % a.n, iw = q / a.n;
    const int64_t S = a.n * a.G, slot0 = i * a.G;
    const bool live = r < nx;

    double np[P];
#pragma unroll
    for (int c = 0; c < P; c++) np[c] = (live && c < nx) ? -a.ab[ab_index(S, slot0, c) + r] : 0.0;
    const double g0 = live ? a.ab[ab_index(S, slot0, a.G + a.iu) + r] : 0.0;
    cv[r] = live ? a.cd[cd_index(a.n, i, a.ny, a.iy, r)] : 0.0;
    const double d = a.cd[cd_index(a.n, i, a.ny, a.iy, nx + a.iu)];
    double pr, pi;
    const bool ok = circle_response<P>(g, np, g0, d, nx, live, pan, xs, cv, a.cs[iw], a.sn[iw], pr, pi);
    if (!valid || r != 0) return;
    const double nan = __builtin_nan("");
    a.re[q] = ok ? pr : nan;
    a.im[q] = ok ? pi : nan;
}

template <int P>
__global__ __launch_bounds__(WAVE) void k_lss_dmargins(DMarginArgs a) {
    constexpr int NG = WAVE / P, PER = 64 / P, KMAX = FB_MARGINS_KMAX;
    constexpr int GD = PANEL<P> + 2 * DM_CHUNKS;   // doubles per group: the panel | the bracket words
    __shared__ __attribute__((aligned(16))) double lds[NG * GD];
    const Lanes<P> g;
    double2* pan = reinterpret_cast<double2*>(lds + (threadIdx.x / P) * GD);
    double2* xs = pan + (P + 1);
    double* cv = reinterpret_cast<double*>(xs + P);
    unsigned long long* msk = reinterpret_cast<unsigned long long*>(cv + P);   // [2 x DM_CHUNKS]: phase, gain
    const int r = g.r, nx = a.nx, nw = a.nw;
    const int64_t n = a.n;
    const int64_t i_own = (int64_t)blockIdx.x * NG + threadIdx.x / P;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const int64_t S = n * a.G, slot0 = i * a.G;
    const bool live = r < nx, store = valid && r == 0;
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    // ---- this lane's row of [-Phi | gamma], c into the panel, d and the gain; whether all of that is finite
    double np[P];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < P; c++) {
        np[c] = (live && c < nx) ? -a.ab[ab_index(S, slot0, c) + r] : 0.0;
        fin = fin && is_fin(np[c]);
    }
    const double g0 = live ? a.ab[ab_index(S, slot0, a.G + a.iu) + r] : 0.0;
    const double c0 = live ? a.cd[cd_index(n, i, a.ny, a.iy, r)] : 0.0;
    const double d = a.cd[cd_index(n, i, a.ny, a.iy, nx + a.iu)];
    const double gn = a.gain ? a.gain[i] : 1.0;
    const bool notfin = g.any(!(fin && is_fin(g0) && is_fin(c0) && is_fin(d) && is_fin(gn)));
    cv[r] = c0;

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
        if (r == 0) { msk[c] = mp; msk[DM_CHUNKS + c] = mg; }
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
    double clo = a.cs[0], slo = a.sn[0], chi = clo, shi = slo, llr = 0.0, lli = 0.0;   // the bracket's ends on the circle and L at lo
    double zpr = nan, zpi = nan, pcr = nan, pci = nan, zgr = nan, zgi = nan, gcr = nan, gci = nan, gnum = 0.0, gden = 1.0;
    auto pending = [&] { return (curp | curg) != 0 || (sump | sumg) != 0; };
    auto before = [&](double lr, double li) { return kind == 0 ? li < 0.0 : mag2(lr, li) < 1.0; };   // the bracket's predicate
    auto pop = [&] {
        kind = (curp != 0 || sump != 0) ? 0 : 1;
        unsigned long long cur = kind == 0 ? curp : curg;
        unsigned sum = kind == 0 ? sump : sumg;
        int cb = kind == 0 ? basep : baseg;
        if (cur == 0) {
            const int c = __builtin_ctz(sum);
            cur = msk[kind * DM_CHUNKS + c];
            sum &= sum - 1;
            cb = 64 * c;
        }
        const int k = cb + __builtin_ctzll(cur);
        cur &= cur - 1;
        if (kind == 0) { curp = cur; sump = sum; basep = cb; } else { curg = cur; sumg = sum; baseg = cb; }
        if (kind == 1 && ngc == KMAX) { trunc = true; curg = 0; sumg = 0; return; }   // (a gain bracket always counts: nothing to refine)
        clo = a.cs[k]; slo = a.sn[k]; chi = a.cs[k + 1]; shi = a.sn[k + 1];
        llr = gn * a.re[(int64_t)k * n + i]; lli = gn * a.im[(int64_t)k * n + i];
        plo = before(llr, lli);
        it = 0; active = true;
    };
    auto record = [&] {
        if (kind == 0) {
            if (!(llr < 0.0)) return;
            if (npc == KMAX) { trunc = true; curp = 0; sump = 0; return; }
            if (npc == 0 || closer_to_one(-llr, -pcr)) { zpr = clo; zpi = slo; pcr = llr; pci = lli; }
        } else {
            // the largest -Re L* / |L*|, as sign(x) x^2 / |L*|^2 by cross-multiplication
            const double num = -llr * fabs(llr), den = mag2(llr, lli);
            const double ours = num * gden, theirs = gnum * den;
            if (ngc == 0 || ours > theirs) { zgr = clo; zgi = slo; gcr = llr; gci = lli; gnum = num; gden = den; }
        }
        const int slot = kind == 0 ? npc : ngc;
        if (a.all && store) {
            const int64_t row = (int64_t)KMAX * n;
            double* q = a.all + ((int64_t)(4 * kind) * KMAX + slot) * n + i;
            q[0] = clo; q[row] = slo; q[2 * row] = llr; q[3 * row] = lli;
        }
        if (kind == 0) npc++; else ngc++;
    };
    for (;;) {
        // a bracket that has ended is recorded and the next one popped in the same trip
        bool step = false;
        double cz = clo, sz = slo;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (!step) {
                if (!active && pending()) pop();
                if (active) {
                    // the midpoint of the arc: (z_lo + z_hi) / |z_lo + z_hi| (two grid points are less than half a turn apart)
                    const double mr = clo + chi, mi = slo + shi;
                    const double inv = 1.0 / sqrt(fma(mr, mr, mi * mi));
                    double cm = mr * inv, sm = mi * inv;
                    // the division's rounding can leave the midpoint of two neighbouring points an ulp outside them, where it never equals
                    // either: each component is held between the ends' where it is monotone along the arc, the cosine on all of (0, pi],
                    // the sine where both ends lie on the same side of pi / 2
                    cm = fmin(fmax(cm, fmin(clo, chi)), fmax(clo, chi));
                    if ((clo >= 0.0) == (chi >= 0.0)) sm = fmin(fmax(sm, fmin(slo, shi)), fmax(slo, shi));
                    const bool end = (cm == clo && sm == slo) || (cm == chi && sm == shi);
                    if (!end && it < DM_ITERS) { step = true; cz = cm; sz = sm; }
                    else { record(); active = false; }
                }
            }
        }
        if (!__any(active || pending())) break;
        double lr, li;
        const bool ok = circle_response<P>(g, np, g0, d, nx, live, pan, xs, cv, cz, sz, lr, li);
        if (step) {
            lr *= gn; li *= gn;
            if (!ok) { sing = true; active = false; curp = curg = 0; sump = sumg = 0; }
            else {
                it++;
                if (before(lr, li) == plo) { clo = cz; slo = sz; llr = lr; lli = li; } else { chi = cz; shi = sz; }
            }
        }
    }

    // ---- what the system leaves: a status that voids it stores NaN and zero counts
    const bool voided = notfin || sing;
    if (a.all && valid) {
        for (int e = r; e < 8 * KMAX; e += P) {
            const int slot = e % KMAX, knd = e / (4 * KMAX);
            if (voided || slot >= (knd == 0 ? npc : ngc)) a.all[(int64_t)e * n + i] = nan;
        }
    }
    if (!store) return;
    const double out[10] = {zpi, zpr, zgi, zgr, pcr, pci, gcr, gci, s2g, ksg < nw ? (double)ksg : nan};
#pragma unroll
    for (int k = 0; k < 10; k++) a.sel[(int64_t)k * n + i] = voided ? nan : out[k];
    a.counts[i] = voided ? 0 : npc;
    a.counts[n + i] = voided ? 0 : ngc;
    a.status[i] = notfin ? FB_MARGINS_NOT_FINITE : sing ? FB_MARGINS_SINGULAR : trunc ? FB_MARGINS_TRUNCATED : 0;
}

}  // namespace fbw
