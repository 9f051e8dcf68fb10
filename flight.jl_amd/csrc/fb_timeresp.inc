// fb_timeresp.inc — step responses and StepInfo of a Model(lss) batch (include/flightbatch.h: fb_lss_stepinfo; kernels: timeresp_kernels.hpp;
// docs/design/linearize.md, "Step responses on the device"). Included by fb_capi.hip after fb_lss.inc (the verbs' shared scaffold).
// Reference: FA design/robot2d/robot2d_design.ipynb calls step(P[:y, :u], t_sim) and stepinfo of it on the velocity loop and on the position
// loop; here one call does so for m channels of every system of a batch, and flightbatch/timeresp.py prints the reference's table.

extern "C" {

int32_t fb_lss_stepinfo_samples(int32_t nsteps, int32_t stride) {
    if (nsteps < 1 || stride < 1) return -1;
    return (int32_t)(((int64_t)nsteps + stride - 1) / stride + 1);
}

int32_t fb_lss_stepinfo(fb_handle h, const int32_t* iu, const int32_t* iy, int32_t m, double t_sim, double dt, const double* opts,
                        const double* y0_in, const double* yf_in, int32_t stride, double* y, double* info, int32_t* status) {
    if (int32_t rc = verb_handle("fb_lss_stepinfo", h, FB_STEPINFO_NX_MAX, "call", "FB_STEPINFO_NX_MAX: one lane of a group of 32 is the output's")) return rc;
    const LssState* L = h->lss;
    if (m < 1 || m > 64) return fail("fb_lss_stepinfo: m = %d, a call takes 1 <= m <= 64 channels", (int)m);
    if (h->n * (int64_t)m > ((int64_t)1 << 31) - 1)
        return fail("fb_lss_stepinfo: %lld systems x %d channels exceed the 2^31 - 1 pairs of one launch grid", (long long)h->n, (int)m);
    if (int32_t rc = verb_model("fb_lss_stepinfo", h)) return rc;
    if (!iu || !iy) return fail("fb_lss_stepinfo: iu and iy are required");
    for (int j = 0; j < m; j++) {
        if (iu[j] < 0 || iu[j] >= L->nu) return fail("fb_lss_stepinfo: iu[%d] = %d is outside [0, %d)", j, (int)iu[j], L->nu);
        if (iy[j] < 0 || iy[j] >= L->ny) return fail("fb_lss_stepinfo: iy[%d] = %d is outside [0, %d)", j, (int)iy[j], L->ny);
    }
    const bool sampled = L->Ts > 0.0;   // (fb_lss_c2d: the samples are the map's, at t_k = k Ts)
    if (sampled) {
        if (dt == 0.0 || !std::isfinite(dt)) dt = L->Ts;
        if (memcmp(&dt, &L->Ts, sizeof(double)) != 0)
            return fail("fb_lss_stepinfo: dt = %.17g on a sampled model with Ts = %.17g (fb_lss_c2d): pass its Ts, or 0 for it", dt, L->Ts);
    }
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail("fb_lss_stepinfo: dt = %g must be positive and finite", dt);
    if (!(t_sim >= dt) || !std::isfinite(t_sim)) return fail("fb_lss_stepinfo: t_sim = %g must be finite and at least dt = %g", t_sim, dt);
    const double steps = std::round(t_sim / dt);
    if (!(steps <= 200000.0)) return fail("fb_lss_stepinfo: t_sim / dt = %g steps, a call takes at most 200000", steps);
    if (stride < 1) return fail("fb_lss_stepinfo: stride = %d must be at least 1", (int)stride);
    const double th = opts ? opts[0] : 0.02, lo = opts ? opts[1] : 0.1, hi = opts ? opts[2] : 0.9;
    if (!(th > 0.0) || !std::isfinite(th)) return fail("fb_lss_stepinfo: settling_th = %g must be positive and finite", th);
    if (!(0.0 < lo && lo < hi && hi < 1.0)) return fail("fb_lss_stepinfo: the rise thresholds (%g, %g) must satisfy 0 < lo < hi < 1", lo, hi);
    if (!info || !status) return fail("fb_lss_stepinfo: info and status are required");
    HIPCHK(hipSetDevice(h->device));
    const int N = (int)steps, ns = fb_lss_stepinfo_samples(N, stride);
    const size_t nc = (size_t)h->n * (size_t)m;
    // one device block: y0_in | yf_in | y | info, then the int32 words status | iu | iy
    const size_t n_y0 = y0_in ? nc : 0, n_yf = yf_in ? nc : 0, n_y = y ? (size_t)ns * nc : 0;
    const size_t nd = n_y0 + n_yf + n_y + 9 * nc, ni = nc + 2 * (size_t)m;
    DevBlocks blocks;
    double* d = nullptr;
    if (int32_t rc = blocks.alloc(&d, nd + (ni + 1) / 2)) return rc;   // (the int32 words behind the doubles)
    double *d_y0 = d, *d_yf = d_y0 + n_y0, *d_y = d_yf + n_yf, *d_info = d_y + n_y;
    int32_t *d_st = reinterpret_cast<int32_t*>(d + nd), *d_iu = d_st + nc, *d_iy = d_iu + m;
    if (y0_in) HIPCHK(hipMemcpyAsync(d_y0, y0_in, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
    if (yf_in) HIPCHK(hipMemcpyAsync(d_yf, yf_in, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_iu, iu, sizeof(int32_t) * m, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_iy, iy, sizeof(int32_t) * m, hipMemcpyHostToDevice, h->stream));
    fbt::TimeRespArgs a = {};
    verb_args(a, h);
    a.iu = d_iu; a.iy = d_iy;
    a.y0_in = y0_in ? d_y0 : nullptr; a.yf_in = yf_in ? d_yf : nullptr; a.y = y ? d_y : nullptr; a.info = d_info; a.status = d_st;
    a.m = m; a.nsteps = N; a.stride = stride; a.ns = ns;
    a.dt = dt; a.settling_th = th; a.rise_lo = lo; a.rise_hi = hi;
    if (!sampled) {
        if (int32_t rc = family_launch(h, group_for(a.nx + 1), (int64_t)nc, a, [](auto P) { return fbt::k_timeresp<P.value>; })) return rc;
    } else if (int32_t rc = family_launch(h, group_for(a.nx + 1), (int64_t)nc, a, [](auto P) { return fbz::k_timeresp_map<P.value>; })) return rc;
    if (y) HIPCHK(hipMemcpyAsync(y, d_y, sizeof(double) * n_y, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(info, d_info, sizeof(double) * 9 * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
