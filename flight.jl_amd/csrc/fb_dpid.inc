// fb_dpid.inc — the metrics of optimize_PID on a SAMPLED Model(lss) batch under the sampled PID law (include/flightbatch.h:
// fb_lss_dpid_metrics; kernels: dpid_kernels.hpp, and fbw::k_lss_dfreqresp for P(z) on the grid; docs/design/linearize.md, "Discrete PID
// design on the device"). Included by fb_capi.hip after fb_dfreq.inc (the d verbs' handle check; the grid check and the sliced grid response are fb_pid.inc's).
// Reference: f_periodic! of PID, FP/control.jl:431-471, is the law Cessna172Xv2 and Robot2D run every dt = 0.02; FA design/pidopt.jl designs
// its gains on the continuous compensator (fb_pid.inc). Here one call evaluates pidopt.jl's metrics of every (system, candidate) pair under
// the law as it runs; the search that proposes the candidates is host-side (flightbatch/dpid.py).
// Every refusal is decided here, before anything is launched.

extern "C" {

int32_t fb_lss_dpid_metrics(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, double t_sim, const double* weights,
                            const double* pid, const double* bounds, int32_t m, double* metrics, double* cost, int32_t* counts, int32_t* status) {
    static const char* verb = "fb_lss_dpid_metrics";
    if (int32_t rc = dverb_handle(verb, h, FB_DPID_NX_MAX, "FB_DPID_NX_MAX")) return rc;
    std::vector<double> cs, sn;
    if (int32_t rc = freq_check_grid(verb, h, iu, iy, w, nw, 1, false, h->lss->Ts, &cs, &sn)) return rc;
    if (m < 1 || m > 64) return fail("%s: m = %d, a call takes 1 <= m <= 64 candidates per system", verb, (int)m);
    if (h->n * (int64_t)m > ((int64_t)1 << 31) - 1)
        return fail("%s: %lld systems x %d candidates exceed the 2^31 - 1 pairs of one launch grid", verb, (long long)h->n, (int)m);
    const double Ts = h->lss->Ts;
    if (!std::isfinite(t_sim)) return fail("%s: t_sim = %g must be finite", verb, t_sim);
    const double ticks = std::round(t_sim / Ts);
    if (!(ticks >= 1.0) || !(ticks <= 200000.0))
        return fail("%s: t_sim / Ts = %g ticks (t_sim = %g, Ts = %g), a call takes 1 <= N <= 200000", verb, ticks, t_sim, Ts);
    if (!pid || !cost || !status) return fail("%s: pid, cost and status are required", verb);
    fbu::DPidArgs a = {};
    for (int k = 0; k < 5; k++) {
        a.wt[k] = weights ? weights[k] : 1.0;
        if (!(a.wt[k] >= 0.0) || !std::isfinite(a.wt[k])) return fail("%s: weights[%d] = %g, a weight must be finite and not negative", verb, k, a.wt[k]);
        a.wsum += a.wt[k];
    }
    if (!(a.wsum > 0.0)) return fail("%s: the weights sum to zero", verb);
    const size_t n = (size_t)h->n, np = n * (size_t)nw, nc = n * (size_t)m;
    for (size_t k = 0; k < nc; k++) {
        const double tf = pid[3 * nc + k];
        if (!(tf >= 0.0) || !std::isfinite(tf))
            return fail("%s: tau_f = %g at system %lld, candidate %lld: the derivative filter's time constant must be finite and not negative",
                        verb, tf, (long long)(k % n), (long long)(k / n));
    }
    for (size_t k = 0; bounds && k < nc; k++) {
        const double lo = bounds[k], hi = bounds[nc + k];
        if (lo != lo || hi != hi || !(lo < hi))
            return fail("%s: bounds lo = %g, hi = %g at system %lld, candidate %lld: the output bounds must satisfy lo < hi (either may be infinite)",
                        verb, lo, hi, (long long)(k % n), (long long)(k / n));
    }
    int64_t slice = 0;
    if (int32_t rc = freq_slice(verb, h, &slice)) return rc;
    HIPCHK(hipSetDevice(h->device));
    // one device block: cos | sin | P(z) re | im | pid | bounds | metrics | cost; counts | status apart
    const size_t nb = bounds ? 2 * nc : 0, nm = metrics ? 5 * nc : 0, nk = counts ? 2 * nc : 0;
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, 2 * (size_t)nw + 2 * np + 4 * nc + nb + nm + nc)) return rc;
    if (int32_t rc = blocks.alloc(&di, nk + nc)) return rc;
    double *d_re = d + 2 * nw, *d_im = d_re + np, *d_pid = d_im + np, *d_bnd = d_pid + 4 * nc, *d_met = d_bnd + nb, *d_cost = d_met + nm;
    HIPCHK(hipMemcpyAsync(d, cs.data(), sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d + nw, sn.data(), sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_pid, pid, sizeof(double) * 4 * nc, hipMemcpyHostToDevice, h->stream));
    if (bounds) HIPCHK(hipMemcpyAsync(d_bnd, bounds, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
    if (int32_t rc = freq_grid(h, iu, iy, d, d + nw, nw, slice, d_re, d_im)) return rc;
    verb_args(a, h);
    a.cs = d; a.sn = d + nw; a.pre = d_re; a.pim = d_im; a.pid = d_pid; a.bounds = bounds ? d_bnd : nullptr;
    a.metrics = metrics ? d_met : nullptr; a.cost = d_cost; a.counts = counts ? di : nullptr; a.status = di + nk;
    a.iu = iu; a.iy = iy; a.nw = nw; a.m = m;
    a.nticks = (int)ticks; a.Ts = Ts;
    if (int32_t rc = family_launch(h, group_for(a.nx + 1), (int64_t)nc, a, [](auto P) { return fbu::k_dpid_metrics<P.value>; })) return rc;
    if (metrics) HIPCHK(hipMemcpyAsync(metrics, d_met, sizeof(double) * nm, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(hipMemcpyAsync(counts, di, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cost, d_cost, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, di + nk, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
