// fb_dfreq.inc — the analysis verbs of sampled Model(lss) batches (include/flightbatch.h: fb_lss_set_sampled, fb_lss_dfreqresp,
// fb_lss_dmargins, fb_lss_dpoles; kernels: dfreq_kernels.hpp, and fbe::k_poles for the poles; docs/design/linearize.md, "Sampled loops on
// the device"). Included by fb_capi.hip after fb_dlqr.inc.
// Reference: the controllers of FP/control.jl run in f_periodic! at dt = 0.02 on gains designed in continuous time; ControlSystems'
// freqresp, margin, poles and damp on a discrete system are what these verbs compute for a batch.
// Every refusal is decided here, before anything is launched. The host forms theta_k = w_k Ts and its cosine and sine with the C library
// (the device library is built with -fapprox-func: no trigonometric function is evaluated on the device), and turns the point z* of a
// crossing back into w* = atan2(Im z*, Re z*) / Ts. The grid check (with Ts: the Nyquist refusal, cos and sin), the sliced grid response and
// the margins' finishing step are the ones the continuous verbs use (fb_pid.inc).

// what the three d verbs ask of their handle: a LinearizedSS handle with a model that is sampled
static int32_t dverb_handle(const char* verb, fb_handle h, int nx_max, const char* limit) {
    if (!h) return fail("%s: null handle", verb);
    if (int32_t rc = verb_handle(verb, h, nx_max, "call", limit)) return rc;
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (!(h->lss->Ts > 0.0)) return fail("%s: a discrete-time verb on a continuous model: sample it first (fb_lss_c2d, or fb_lss_set_sampled on a model that holds Phi and Gamma)", verb);
    return 0;
}

extern "C" {

int32_t fb_lss_set_sampled(fb_handle h, double Ts) {
    static const char* verb = "fb_lss_set_sampled";
    if (!h) return fail("%s: null handle", verb);
    if (!is_lss(h)) return fail("%s: the handle is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)", verb);
    if (!h->lss) return fail("%s: the handle is not ready (its creation did not finish)", verb);
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (h->lss->Ts > 0.0) return fail("%s: the handle is already a sampled model (Ts = %g)", verb, h->lss->Ts);
    if (!(Ts > 0.0) || !std::isfinite(Ts)) return fail("%s: Ts = %g must be positive and finite", verb, Ts);
    h->lss->Ts = Ts;          // sampled: A's place is read as Phi, B's as Gamma, xdot0's as delta (where fb_lss_c2d leaves them)
    h->params.dt = Ts;
    return 0;
}

int32_t fb_lss_dfreqresp(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, double* re, double* im) {
    static const char* verb = "fb_lss_dfreqresp";
    if (int32_t rc = dverb_handle(verb, h, FB_MARGINS_NX_MAX, "FB_MARGINS_NX_MAX")) return rc;
    std::vector<double> cs, sn;
    if (int32_t rc = freq_check_grid(verb, h, iu, iy, w, nw, 1, false, h->lss->Ts, &cs, &sn)) return rc;
    if (!re || !im) return fail("%s: re and im are required", verb);
    int64_t slice = 0;
    if (int32_t rc = freq_slice(verb, h, &slice)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = n * (size_t)nw;
    DevBlocks blocks;
    double* d = nullptr;   // one device block: cos | sin | re | im
    if (int32_t rc = blocks.alloc(&d, 2 * (size_t)nw + 2 * np)) return rc;
    double *d_re = d + 2 * nw, *d_im = d_re + np;
    HIPCHK(hipMemcpyAsync(d, cs.data(), sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d + nw, sn.data(), sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    if (int32_t rc = freq_grid(h, iu, iy, d, d + nw, nw, slice, d_re, d_im)) return rc;
    HIPCHK(hipMemcpyAsync(re, d_re, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(im, d_im, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int32_t fb_lss_dmargins(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, const double* gain, double* sel, int32_t* counts,
                        double* all, int32_t* status) {
    static const char* verb = "fb_lss_dmargins";
    if (int32_t rc = dverb_handle(verb, h, FB_MARGINS_NX_MAX, "FB_MARGINS_NX_MAX")) return rc;
    std::vector<double> cs, sn;
    if (int32_t rc = freq_check_grid(verb, h, iu, iy, w, nw, 2, true, h->lss->Ts, &cs, &sn)) return rc;
    if (!sel || !counts || !status) return fail("%s: sel, counts and status are required", verb);
    if (int32_t rc = freq_check_pairs(verb, h, nw)) return rc;
    int64_t slice = 0;
    if (int32_t rc = freq_slice(verb, h, &slice)) return rc;

    HIPCHK(hipSetDevice(h->device));
    const double Ts = h->lss->Ts;
    const size_t n = (size_t)h->n, np = n * (size_t)nw, K = FB_MARGINS_KMAX, na = all ? 8 * K * n : 0;
    // one device block: cos | sin | L re | im | gain | sel | all (the device's eight rows a slot); counts | status apart
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, 2 * (size_t)nw + 2 * np + n + 10 * n + na)) return rc;
    if (int32_t rc = blocks.alloc(&di, 3 * n)) return rc;
    double *d_re = d + 2 * nw, *d_im = d_re + np, *d_gain = d_im + np, *d_sel = d_gain + n, *d_all = d_sel + 10 * n;
    HIPCHK(hipMemcpyAsync(d, cs.data(), sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d + nw, sn.data(), sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    if (gain) HIPCHK(hipMemcpyAsync(d_gain, gain, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    if (int32_t rc = freq_grid(h, iu, iy, d, d + nw, nw, slice, d_re, d_im)) return rc;
    fbw::DMarginArgs a = {};
    verb_args(a, h);
    a.cs = d; a.sn = d + nw; a.re = d_re; a.im = d_im; a.gain = gain ? d_gain : nullptr;
    a.sel = d_sel; a.all = all ? d_all : nullptr; a.counts = di; a.status = di + 2 * n;
    a.iu = iu; a.iy = iy; a.nw = nw;
    if (int32_t rc = family_launch(h, group_for(a.nx), h->n, a, [](auto P) { return fbw::k_lss_dmargins<P.value>; })) return rc;
    std::vector<double> every(na);
    HIPCHK(hipMemcpyAsync(sel, d_sel, sizeof(double) * 10 * n, hipMemcpyDeviceToHost, h->stream));
    if (all) HIPCHK(hipMemcpyAsync(every.data(), d_all, sizeof(double) * na, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(counts, di, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, di + 2 * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    // w* from the point of the circle (the host's atan2) around the finishing step, and the grid frequency of smin from its index
    const double nan = std::nan("");
    for (size_t i = 0; i < n; i++) {
        const double wpc = counts[i] ? std::atan2(sel[i], sel[n + i]) / Ts : nan;
        const double wgc = counts[n + i] ? std::atan2(sel[2 * n + i], sel[3 * n + i]) / Ts : nan;
        if (!margins_finish(sel, counts, status, n, i)) continue;
        sel[n + i] = wpc;
        sel[3 * n + i] = wgc;
        const double ks = sel[9 * n + i];
        sel[9 * n + i] = ks >= 0.0 && ks < (double)nw ? w[(int)ks] : nan;
    }
    // the device's rows Re z*, Im z*, Re L*, Im L* of a kind into the ABI's w*, Re L*, Im L* (NaN past the count stays NaN)
    for (size_t kind = 0; all && kind < 2; kind++)
        for (size_t s = 0; s < K; s++)
            for (size_t i = 0; i < n; i++) {
                const double* q = every.data() + (4 * kind * K + s) * n + i;
                double* o = all + (3 * kind * K + s) * n + i;
                o[0] = std::atan2(q[K * n], q[0]) / Ts;
                o[K * n] = q[2 * K * n];
                o[2 * K * n] = q[3 * K * n];
            }
    return 0;
}

int32_t fb_lss_dpoles(fb_handle h, double* re, double* im, int32_t* iters, int32_t* status) {
    if (int32_t rc = dverb_handle("fb_lss_dpoles", h, FB_POLES_NX_MAX, "FB_POLES_NX_MAX")) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = (size_t)h->lss->nx * n;
    // one device block: re | im; iters, status apart. The eigenvalues of what stands in A's place: Phi
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, 2 * np)) return rc;
    if (int32_t rc = blocks.alloc(&di, 2 * n)) return rc;
    fbe::PolesArgs a = {};
    verb_args_ab(a, h);
    a.re = d; a.im = d + np; a.iters = di; a.status = di + n;
    if (int32_t rc = family_launch(h, group_for(a.nx), h->n, a, [](auto P) { return fbe::k_poles<P.value>; })) return rc;
    if (re) HIPCHK(hipMemcpyAsync(re, a.re, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    if (im) HIPCHK(hipMemcpyAsync(im, a.im, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    if (iters) HIPCHK(hipMemcpyAsync(iters, a.iters, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
