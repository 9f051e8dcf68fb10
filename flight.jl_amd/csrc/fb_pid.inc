// fb_pid.inc — the metrics of optimize_PID on a Model(lss) batch (include/flightbatch.h: fb_lss_freqresp, fb_pid_metrics; kernels:
// pid_kernels.hpp; docs/design/linearize.md, "PID loop design on the device"). Included by fb_capi.hip after fb_lss.inc (the verbs' shared scaffold).
// Reference: FA design/pidopt.jl — Metrics(plant, pid, settings) :36-64 and cost :66-70 are what optimize_PID :73-128 evaluates up to 5000
// times per design node (design/c172/c172x_design.jl:236, 279, 309, 717, 746). Here one call evaluates every (system, candidate) pair of
// a batch; the search that proposes the candidates is host-side (flightbatch/pidopt.py).

// what both entry points ask of the handle, the channel and the grid; nothing has touched a device when this refuses
static int32_t pid_check_plant(const char* verb, fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw) {
    if (int32_t rc = verb_handle(verb, h, FB_PID_NX_MAX, "design", "FB_PID_NX_MAX")) return rc;
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (int32_t rc = verb_continuous(verb, h)) return rc;
    const LssState* L = h->lss;
    if (iu < 0 || iu >= L->nu) return fail("%s: iu = %d is outside [0, %d)", verb, (int)iu, L->nu);
    if (iy < 0 || iy >= L->ny) return fail("%s: iy = %d is outside [0, %d)", verb, (int)iy, L->ny);
    if (!w) return fail("%s: the frequency grid w is required", verb);
    if (nw < 1 || nw > 1024) return fail("%s: nw = %d, the grid takes 1 <= nw <= 1024 frequencies", verb, (int)nw);
    for (int k = 0; k < nw; k++)
        if (!(w[k] > 0.0) || !std::isfinite(w[k])) return fail("%s: w[%d] = %g, every frequency must be positive and finite", verb, k, w[k]);
    if (h->n * (int64_t)nw > ((int64_t)1 << 31) - 1)
        return fail("%s: %lld systems x %d frequencies exceed the 2^31 - 1 pairs of one launch grid", verb, (long long)h->n, (int)nw);
    return 0;
}

// k_lss_freqresp of channel (iu, iy) on the grid d_w [nw] (device) into re, im [nw x n] (device)
static int32_t pid_freqresp(fb_handle h, int32_t iu, int32_t iy, const double* d_w, int32_t nw, double* re, double* im) {
    fbp::FreqArgs a = {};
    verb_args(a, h);
    a.w = d_w; a.re = re; a.im = im; a.iu = iu; a.iy = iy; a.nw = nw;
    return family_launch(h, group_for(a.nx), a.n * a.nw, a, [](auto P) { return fbp::k_lss_freqresp<P.value>; });
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
    if (int32_t rc = pid_freqresp(h, iu, iy, d, nw, d + nw, d + nw + np)) return rc;
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
    if (int32_t rc = pid_freqresp(h, iu, iy, d, nw, d_re, d_im)) return rc;
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
