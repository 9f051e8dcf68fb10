// fb_pid.inc — the metrics of optimize_PID on a Model(lss) batch (include/flightbatch.h: fb_lss_freqresp, fb_pid_metrics; kernels:
// pid_kernels.hpp; docs/design/linearize.md, "PID loop design on the device"). Included by fb_capi.hip after fb_lss.inc (the verbs' shared scaffold).
// Reference: FA design/pidopt.jl — Metrics(plant, pid, settings) :36-64 and cost :66-70 are what optimize_PID :73-128 evaluates up to 5000
// times per design node (design/c172/c172x_design.jl:236, 279, 309, 717, 746). Here one call evaluates every (system, candidate) pair of
// a batch; the search that proposes the candidates is host-side (flightbatch/pidopt.py).

// ---- what the frequency-domain verbs of both time domains share on the host (fb_lss_freqresp, fb_pid_metrics, fb_lss_margins; fb_lss_dfreqresp,
// fb_lss_dmargins, fb_lss_dpid_metrics). Every refusal is decided before anything has touched a device.

// the channel and the grid. Ts = 0: a continuous model; otherwise a sampled one: no frequency above the Nyquist frequency, and cs, sn are
// filled with cos and sin of theta_k = w_k Ts. `increasing`: the margins' grids
static int32_t freq_check_grid(const char* verb, fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, int nw_min, bool increasing,
                               double Ts, std::vector<double>* cs, std::vector<double>* sn) {
    const LssState* L = h->lss;
    const double pi = 3.14159265358979323846;
    const bool sampled = Ts > 0.0;
    if (iu < 0 || iu >= L->nu) return fail("%s: iu = %d is outside [0, %d)", verb, (int)iu, L->nu);
    if (iy < 0 || iy >= L->ny) return fail("%s: iy = %d is outside [0, %d)", verb, (int)iy, L->ny);
    if (!w) return fail("%s: the frequency grid w is required", verb);
    if (nw < nw_min || nw > 1024) return fail("%s: nw = %d, the grid takes %d <= nw <= 1024 frequencies", verb, (int)nw, nw_min);
    if (sampled) { cs->resize(nw); sn->resize(nw); }
    double before = 0.0;
    for (int k = 0; k < nw; k++) {
        if (!(w[k] > 0.0) || !std::isfinite(w[k])) return fail("%s: w[%d] = %g, every frequency must be positive and finite", verb, k, w[k]);
        const double th = sampled ? w[k] * Ts : w[k];
        if (sampled && !(th <= pi)) return fail("%s: w[%d] = %.17g is above the Nyquist frequency pi/Ts = %.17g (Ts = %g)", verb, k, w[k], pi / Ts, Ts);
        if (increasing && k > 0 && !(th > before))
            return fail("%s: w[%d] = %g after w[%d] = %g, the grid%s must strictly increase", verb, k, w[k], k - 1, w[k - 1], sampled ? "'s angles w Ts" : "");
        before = th;
        if (sampled) { (*cs)[k] = std::cos(th); (*sn)[k] = std::sin(th); }
    }
    return 0;
}

// the verbs whose kernels index the whole grid of the batch with an int
static int32_t freq_check_pairs(const char* verb, fb_handle h, int32_t nw) {
    if (h->n * (int64_t)nw > ((int64_t)1 << 31) - 1)
        return fail("%s: %lld systems x %d frequencies exceed the 2^31 - 1 pairs of one launch grid", verb, (long long)h->n, (int)nw);
    return 0;
}

// The grid response runs in slices of whole frequencies: a launch of one-wave workgroups holds fewer than 2^32 lanes, and N nw / (64 / P)
// workgroups of a grid kernel pass that at a million systems on the default grid once P > 8. A slice is a contiguous block of re and im (the
// system index is the fastest), every (system, frequency) pair is computed by the same code as in one launch, and small batches take one slice.
constexpr int64_t FREQ_WG_MAX = (int64_t)1 << 25;   // one-wave workgroups per launch: half of what 2^32 lanes allow

// frequencies per launch of the grid response, refused when one frequency of the batch does not fit a launch
static int32_t freq_slice(const char* verb, fb_handle h, int64_t* slice) {
    const int ng = fbg::WAVE / group_for(h->lss->nx);
    *slice = FREQ_WG_MAX * ng / h->n;
    if (*slice < 1) return fail("%s: %lld systems exceed the %lld one launch of the grid response takes at nx = %d", verb, (long long)h->n,
                                (long long)(FREQ_WG_MAX * ng), h->lss->nx);
    return 0;
}

// the grid response of channel (iu, iy) into re, im [nw x n] (device), `slice` frequencies to a launch: k_lss_freqresp on the frequencies
// d_w [nw] (device) where d_sn is null, k_lss_dfreqresp on the points d_w = cos, d_sn = sin of the circle otherwise
static int32_t freq_grid(fb_handle h, int32_t iu, int32_t iy, const double* d_w, const double* d_sn, int32_t nw, int64_t slice, double* re, double* im) {
    for (int64_t k0 = 0; k0 < nw; k0 += slice) {
        auto window = [&](auto& a) {
            verb_args(a, h);
            a.re = re + k0 * h->n; a.im = im + k0 * h->n;
            a.iu = iu; a.iy = iy; a.nw = (int)std::min<int64_t>(slice, nw - k0);
        };
        int32_t rc;
        if (d_sn) {
            fbw::DFreqArgs a = {};
            window(a);
            a.cs = d_w + k0; a.sn = d_sn + k0;
            rc = family_launch(h, group_for(a.nx), a.n * a.nw, a, [](auto P) { return fbw::k_lss_dfreqresp<P.value>; });
        } else {
            fbp::FreqArgs a = {};
            window(a);
            a.w = d_w + k0;
            rc = family_launch(h, group_for(a.nx), a.n * a.nw, a, [](auto P) { return fbp::k_lss_freqresp<P.value>; });
        }
        if (rc) return rc;
    }
    return 0;
}

// gm, pm and smin of system i from what a margins kernel selected: the host's division, atan2 and sqrt (the device library is built with
// -fapprox-func). False, and nothing done, for a voided system (the kernel stored NaN in every row).
static bool margins_finish(double* sel, const int32_t* counts, const int32_t* status, size_t n, size_t i) {
    if (status[i] & (FB_MARGINS_NOT_FINITE | FB_MARGINS_SINGULAR)) return false;
    const double inf = HUGE_VAL, deg = 180.0 / 3.14159265358979323846;
    sel[i] = counts[i] ? -1.0 / sel[4 * n + i] : inf;
    sel[2 * n + i] = counts[n + i] ? std::atan2(-sel[7 * n + i], -sel[6 * n + i]) * deg : inf;
    sel[8 * n + i] = std::sqrt(sel[8 * n + i]);
    return true;
}

// what both PID entry points ask of the handle, the channel and the grid
static int32_t pid_check_plant(const char* verb, fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw) {
    if (int32_t rc = verb_handle(verb, h, FB_PID_NX_MAX, "design", "FB_PID_NX_MAX")) return rc;
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (int32_t rc = verb_continuous(verb, h)) return rc;
    if (int32_t rc = freq_check_grid(verb, h, iu, iy, w, nw, 1, false, 0.0, nullptr, nullptr)) return rc;
    return freq_check_pairs(verb, h, nw);
}

extern "C" {

int32_t fb_lss_freqresp(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, double* re, double* im) {
    if (int32_t rc = pid_check_plant("fb_lss_freqresp", h, iu, iy, w, nw)) return rc;
    if (!re || !im) return fail("fb_lss_freqresp: re and im are required");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = n * (size_t)nw;
    DevBlocks blocks;
    double* d = nullptr;   // one device block: w | re | im
    if (int32_t rc = blocks.alloc(&d, (size_t)nw + 2 * np)) return rc;
    HIPCHK(hipMemcpyAsync(d, w, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    if (int32_t rc = freq_grid(h, iu, iy, d, nullptr, nw, nw, d + nw, d + nw + np)) return rc;
    HIPCHK(hipMemcpyAsync(re, d + nw, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(im, d + nw + np, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int32_t fb_pid_metrics(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, double t_sim, double dt, const double* weights,
                       const double* pid, int32_t m, double* metrics, double* cost, int32_t* status) {
    if (int32_t rc = pid_check_plant("fb_pid_metrics", h, iu, iy, w, nw)) return rc;
    if (m < 1 || m > 64) return fail("fb_pid_metrics: m = %d, a call takes 1 <= m <= 64 candidates per system", (int)m);
    if (h->n * (int64_t)m > ((int64_t)1 << 31) - 1)
        return fail("fb_pid_metrics: %lld systems x %d candidates exceed the 2^31 - 1 pairs of one launch grid", (long long)h->n, (int)m);
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail("fb_pid_metrics: dt = %g must be positive and finite", dt);
    if (!(t_sim >= dt) || !std::isfinite(t_sim)) return fail("fb_pid_metrics: t_sim = %g must be finite and at least dt = %g", t_sim, dt);
    const double steps = std::round(t_sim / dt);
    if (!(steps <= 200000.0)) return fail("fb_pid_metrics: t_sim / dt = %g steps, a call takes at most 200000", steps);
    if (!pid || !cost || !status) return fail("fb_pid_metrics: pid, cost and status are required");
    fbp::PidArgs a = {};
    for (int k = 0; k < 5; k++) {
        a.wt[k] = weights ? weights[k] : 1.0;
        if (!(a.wt[k] >= 0.0) || !std::isfinite(a.wt[k])) return fail("fb_pid_metrics: weights[%d] = %g, a weight must be finite and not negative", k, a.wt[k]);
        a.wsum += a.wt[k];
    }
    if (!(a.wsum > 0.0)) return fail("fb_pid_metrics: the weights sum to zero");
    const size_t n = (size_t)h->n, np = n * (size_t)nw, nc = n * (size_t)m;
    for (size_t k = 0; k < nc; k++)
        if (!(pid[3 * nc + k] > 0.0) || !std::isfinite(pid[3 * nc + k]))
            return fail("fb_pid_metrics: tau_f = %g at system %lld, candidate %lld: the derivative filter's time constant must be positive",
                        pid[3 * nc + k], (long long)(k % n), (long long)(k / n));
    HIPCHK(hipSetDevice(h->device));
    // one device block: w | P(jw) re | im | pid | metrics | cost; status apart
    const size_t nm = metrics ? 5 * nc : 0;
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, (size_t)nw + 2 * np + 4 * nc + nm + nc)) return rc;
    if (int32_t rc = blocks.alloc(&di, nc)) return rc;
    double *d_re = d + nw, *d_im = d_re + np, *d_pid = d_im + np, *d_met = d_pid + 4 * nc, *d_cost = d_met + nm;
    HIPCHK(hipMemcpyAsync(d, w, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_pid, pid, sizeof(double) * 4 * nc, hipMemcpyHostToDevice, h->stream));
    if (int32_t rc = freq_grid(h, iu, iy, d, nullptr, nw, nw, d_re, d_im)) return rc;
    verb_args(a, h);
    a.w = d; a.pre = d_re; a.pim = d_im; a.pid = d_pid;
    a.metrics = metrics ? d_met : nullptr; a.cost = d_cost; a.status = di;
    a.iu = iu; a.iy = iy; a.nw = nw; a.m = m;
    a.nsteps = (int)steps; a.dt = dt;
    if (int32_t rc = family_launch(h, group_for(a.nx + 4), (int64_t)nc, a, [](auto P) { return fbp::k_pid_metrics<P.value>; })) return rc;
    if (metrics) HIPCHK(hipMemcpyAsync(metrics, d_met, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cost, d_cost, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, di, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
