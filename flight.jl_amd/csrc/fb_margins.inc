// fb_margins.inc — gain and phase margins of a Model(lss) batch (include/flightbatch.h: fb_lss_margins; kernel: margins_kernels.hpp;
// docs/design/linearize.md, "Margins on the device"). Included by fb_capi.hip after fb_pid.inc, whose pid_freqresp is stage 1.
// Reference: FA design/robot2d/robot2d_design.ipynb — marginplot on the position plant and on the position loop with k_p = 0.6.
// Every refusal is decided here, before anything is launched. Stage 1 is called past pid_check_plant: that check holds the PID verbs to
// nx <= FB_PID_NX_MAX (k_pid_metrics needs four lanes beyond the plant's), k_lss_freqresp itself serves every nx group_for does.
// Stage 1 runs in slices of whole frequencies: a launch of one-wave workgroups holds fewer than 2^32 lanes, and N nw / (64 / P) workgroups
// of k_lss_freqresp pass that at a million systems on the default grid once P > 8. A slice is a contiguous block of re and im (the system
// index is the fastest), every (system, frequency) pair is computed by the same code as in one launch, and small batches take one slice.
constexpr int64_t MARGINS_WG_MAX = (int64_t)1 << 25;   // one-wave workgroups per launch: half of what 2^32 lanes allow

extern "C" {

int32_t fb_lss_margins(fb_handle h, int32_t iu, int32_t iy, const double* w, int32_t nw, const double* gain, double* sel, int32_t* counts,
                       double* all, int32_t* status) {
    static const char* verb = "fb_lss_margins";
    if (int32_t rc = verb_handle(verb, h, FB_MARGINS_NX_MAX, "margins", "FB_MARGINS_NX_MAX")) return rc;
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (int32_t rc = verb_continuous(verb, h)) return rc;
    const LssState* L = h->lss;
    if (iu < 0 || iu >= L->nu) return fail("%s: iu = %d is outside [0, %d)", verb, (int)iu, L->nu);
    if (iy < 0 || iy >= L->ny) return fail("%s: iy = %d is outside [0, %d)", verb, (int)iy, L->ny);
    if (!w) return fail("%s: the frequency grid w is required", verb);
    if (!sel || !counts || !status) return fail("%s: sel, counts and status are required", verb);
    if (nw < 2 || nw > 1024) return fail("%s: nw = %d, the grid takes 2 <= nw <= 1024 frequencies", verb, (int)nw);
    for (int k = 0; k < nw; k++) {
        if (!(w[k] > 0.0) || !std::isfinite(w[k])) return fail("%s: w[%d] = %g, every frequency must be positive and finite", verb, k, w[k]);
        if (k > 0 && !(w[k] > w[k - 1])) return fail("%s: w[%d] = %g after w[%d] = %g, the grid must strictly increase", verb, k, w[k], k - 1, w[k - 1]);
    }
    if (h->n * (int64_t)nw > ((int64_t)1 << 31) - 1)
        return fail("%s: %lld systems x %d frequencies exceed the 2^31 - 1 pairs of one launch grid", verb, (long long)h->n, (int)nw);
    const int64_t slice = MARGINS_WG_MAX * (fbg::WAVE / group_for(L->nx)) / h->n;   // frequencies per launch of stage 1
    if (slice < 1) return fail("%s: %lld systems exceed the %lld one launch of the grid response takes at nx = %d", verb, (long long)h->n,
                               (long long)(MARGINS_WG_MAX * (fbg::WAVE / group_for(L->nx))), L->nx);

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
    for (int64_t k0 = 0; k0 < nw; k0 += slice)
        if (int32_t rc = pid_freqresp(h, iu, iy, d + k0, (int32_t)std::min<int64_t>(slice, nw - k0), d_re + k0 * n, d_im + k0 * n)) return rc;
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
    // gm, pm and smin from what the kernel selected: the host's division, atan2 and sqrt (the device library is built with -fapprox-func)
    const double inf = HUGE_VAL, deg = 180.0 / 3.14159265358979323846;
    for (size_t i = 0; i < n; i++) {
        if (status[i] & (FB_MARGINS_NOT_FINITE | FB_MARGINS_SINGULAR)) continue;   // (the kernel stored NaN in every row)
        sel[i] = counts[i] ? -1.0 / sel[4 * n + i] : inf;
        sel[2 * n + i] = counts[n + i] ? std::atan2(-sel[7 * n + i], -sel[6 * n + i]) * deg : inf;
        sel[8 * n + i] = std::sqrt(sel[8 * n + i]);
    }
    return 0;
}

}  // extern "C"
