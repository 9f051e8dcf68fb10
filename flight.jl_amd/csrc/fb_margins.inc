// fb_margins.inc — gain and phase margins of a Model(lss) batch (include/flightbatch.h: fb_lss_margins; kernel: margins_kernels.hpp;
// docs/design/linearize.md, "Margins on the device"). Included by fb_capi.hip after fb_pid.inc, which holds what the frequency-domain verbs
// share on the host: the grid check, the sliced grid response (stage 1) and the finishing step.
// Reference: FA design/robot2d/robot2d_design.ipynb — marginplot on the position plant and on the position loop with k_p = 0.6.
// Every refusal is decided here, before anything is launched. Stage 1 is called past pid_check_plant: that check holds the PID verbs to
// nx <= FB_PID_NX_MAX (k_pid_metrics needs four lanes beyond the plant's), k_lss_freqresp itself serves every nx group_for does.

extern "C" {

int32_t fb_lss_margins(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, const double* gain, double* sel, int32_t* counts,
                       double* all, int32_t* status) {
    static const char* verb = "fb_lss_margins";
    if (int32_t rc = verb_handle(verb, h, FB_MARGINS_NX_MAX, "margins", "FB_MARGINS_NX_MAX")) return rc;
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (int32_t rc = verb_continuous(verb, h)) return rc;
    if (int32_t rc = freq_check_grid(verb, h, iu, iy, w, nw, 2, true, 0.0, nullptr, nullptr)) return rc;
    if (!sel || !counts || !status) return fail("%s: sel, counts and status are required", verb);
    if (int32_t rc = freq_check_pairs(verb, h, nw)) return rc;
    int64_t slice = 0;
    if (int32_t rc = freq_slice(verb, h, &slice)) return rc;

    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = n * (size_t)nw, na = all ? 6 * (size_t)FB_MARGINS_KMAX * n : 0;
    // one device block: w | L re | im | gain | sel | all; counts | status apart
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, (size_t)nw + 2 * np + n + 10 * n + na)) return rc;
    if (int32_t rc = blocks.alloc(&di, 3 * n)) return rc;
    double *d_re = d + nw, *d_im = d_re + np, *d_gain = d_im + np, *d_sel = d_gain + n, *d_all = d_sel + 10 * n;
    HIPCHK(hipMemcpyAsync(d, w, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
    if (gain) HIPCHK(hipMemcpyAsync(d_gain, gain, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    if (int32_t rc = freq_grid(h, iu, iy, d, nullptr, nw, slice, d_re, d_im)) return rc;
    fbn::MarginArgs a = {};
    verb_args(a, h);
    a.w = d; a.re = d_re; a.im = d_im; a.gain = gain ? d_gain : nullptr;
    a.sel = d_sel; a.all = all ? d_all : nullptr; a.counts = di; a.status = di + 2 * n;
    a.iu = iu; a.iy = iy; a.nw = nw;
    if (int32_t rc = family_launch(h, group_for(a.nx), h->n, a, [](auto P) { return fbn::k_lss_margins<P.value>; })) return rc;
    HIPCHK(hipMemcpyAsync(sel, d_sel, sizeof(double) * 10 * n, hipMemcpyDeviceToHost, h->stream));
    if (all) HIPCHK(hipMemcpyAsync(all, d_all, sizeof(double) * na, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(counts, di, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, di + 2 * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++) margins_finish(sel, counts, status, n, i);
    return 0;
}

}  // extern "C"
