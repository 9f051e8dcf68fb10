// fb_pid.inc — the metrics of optimize_PID on a Model(lss) batch (include/flightbatch.h: fb_lss_freqresp, fb_pid_metrics; kernels:
// pid_kernels.hpp; docs/design/linearize.md, "PID loop design on the device"). Included by fb_capi.hip after fb_lqr.inc.
// Reference: FA design/pidopt.jl — Metrics(plant, pid, settings) :36-64 and cost :66-70 are what optimize_PID :73-128 evaluates up to 5000
// times per design node (design/c172/c172x_design.jl:236, 279, 309, 717, 746). Here one call evaluates every (system, candidate) pair of
// a batch; the search that proposes the candidates is host-side (flightbatch/pidopt.py).

static int pid_group(int rows) { return rows <= 8 ? 8 : rows <= 16 ? 16 : 32; }

// what both entry points ask of the handle, the channel and the grid; nothing has touched a device when this refuses
static int32_t pid_check_plant(const char* verb, fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw) {
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("%s: the handle is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)", verb);
    const LssState* L = h->lss;
    if (L->nx > FB_PID_NX_MAX) return fail("%s: nx = %d, the design takes 1 <= nx <= %d (FB_PID_NX_MAX)", verb, L->nx, (int)FB_PID_NX_MAX);
    if (!L->have_model) return fail("%s: this LinearizedSS handle has no model yet (fb_lss_set_model)", verb);
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

static fbp::FreqArgs pid_freq_args(fb_handle h, int32_t iu, int32_t iy, const double* d_w, int32_t nw, double* re, double* im) {
    const LssState* L = h->lss;
    fbp::FreqArgs a = {};
    a.ab = L->ab; a.cd = L->cd; a.w = d_w; a.re = re; a.im = im;
    a.n = h->n; a.nx = L->nx; a.nu = L->nu; a.ny = L->ny; a.G = L->G; a.iu = iu; a.iy = iy; a.nw = nw;
    return a;
}
// k_lss_freqresp on the handle's stream, between a pair of per-launch timing stamps when those are on
static int32_t pid_launch_freqresp(fb_handle h, const fbp::FreqArgs& a) {
    const int P = pid_group(a.nx);
    const dim3 grid = grid_for(a.n * a.nw, fbp::PID_WAVE / P), block(fbp::PID_WAVE);
    const bool stamp = h->timing && h->lev_used < h->lev_max;
    if (stamp) HIPCHK(hipEventRecord(h->lev[2 * h->lev_used], h->stream));
    if (P == 8) hipLaunchKernelGGL(fbp::k_lss_freqresp<8>, grid, block, 0, h->stream, a);
    else if (P == 16) hipLaunchKernelGGL(fbp::k_lss_freqresp<16>, grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL(fbp::k_lss_freqresp<32>, grid, block, 0, h->stream, a);
    if (stamp) { HIPCHK(hipEventRecord(h->lev[2 * h->lev_used + 1], h->stream)); h->lev_used++; }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {

int32_t fb_lss_freqresp(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, double* re, double* im) {
    if (int32_t rc = pid_check_plant("fb_lss_freqresp", h, iu, iy, w, nw)) return rc;
    if (!re || !im) return fail("fb_lss_freqresp: re and im are required");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = n * (size_t)nw;
    double* d = nullptr;   // one device block: w | re | im
    HIPCHK(hipMalloc(&d, sizeof(double) * ((size_t)nw + 2 * np)));
    auto run = [&]() -> int32_t {
        HIPCHK(hipMemcpyAsync(d, w, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
        if (int32_t rc = pid_launch_freqresp(h, pid_freq_args(h, iu, iy, d, nw, d + nw, d + nw + np))) return rc;
        HIPCHK(hipMemcpyAsync(re, d + nw, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(im, d + nw + np, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return 0;
    };
    const int32_t rc = run();
    const std::string msg = g_err;
    (void)hipFree(d);
    g_err = msg;
    return rc;
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
    const LssState* L = h->lss;
    // one device block: w | P(jw) re | im | pid | metrics | cost; status apart
    const size_t nm = metrics ? 5 * nc : 0;
    double* d = nullptr;
    int32_t* di = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(double) * ((size_t)nw + 2 * np + 4 * nc + nm + nc)));
    auto run = [&]() -> int32_t {
        HIPCHK(hipMalloc(&di, sizeof(int32_t) * nc));
        double *d_re = d + nw, *d_im = d_re + np, *d_pid = d_im + np, *d_met = d_pid + 4 * nc, *d_cost = d_met + nm;
        HIPCHK(hipMemcpyAsync(d, w, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_pid, pid, sizeof(double) * 4 * nc, hipMemcpyHostToDevice, h->stream));
        if (int32_t rc = pid_launch_freqresp(h, pid_freq_args(h, iu, iy, d, nw, d_re, d_im))) return rc;
        a.ab = L->ab; a.cd = L->cd; a.w = d; a.pre = d_re; a.pim = d_im; a.pid = d_pid;
        a.metrics = metrics ? d_met : nullptr; a.cost = d_cost; a.status = di;
        a.n = h->n; a.nx = L->nx; a.nu = L->nu; a.ny = L->ny; a.G = L->G; a.iu = iu; a.iy = iy; a.nw = nw; a.m = m;
        a.nsteps = (int)steps; a.dt = dt;
        const int P = pid_group(L->nx + 4);
        const dim3 grid = grid_for((int64_t)nc, fbp::PID_WAVE / P), block(fbp::PID_WAVE);
        const bool stamp = h->timing && h->lev_used < h->lev_max;
        if (stamp) HIPCHK(hipEventRecord(h->lev[2 * h->lev_used], h->stream));
        if (P == 8) hipLaunchKernelGGL(fbp::k_pid_metrics<8>, grid, block, 0, h->stream, a);
        else if (P == 16) hipLaunchKernelGGL(fbp::k_pid_metrics<16>, grid, block, 0, h->stream, a);
        else hipLaunchKernelGGL(fbp::k_pid_metrics<32>, grid, block, 0, h->stream, a);
        if (stamp) { HIPCHK(hipEventRecord(h->lev[2 * h->lev_used + 1], h->stream)); h->lev_used++; }
        HIPCHK(hipGetLastError());
        if (metrics) HIPCHK(hipMemcpyAsync(metrics, d_met, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(cost, d_cost, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(status, di, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return 0;
    };
    const int32_t rc = run();
    const std::string msg = g_err;
    (void)hipFree(d); (void)hipFree(di);
    g_err = msg;
    return rc;
}

}  // extern "C"
