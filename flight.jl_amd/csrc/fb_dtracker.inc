// fb_dtracker.inc — the sampled LQR tracker law on a SAMPLED Model(lss) batch, and the steady-state map of a sampled model
// (include/flightbatch.h: fb_lss_dtracker_metrics, fb_lss_dsteady; kernels: dtracker_kernels.hpp, k_dsteady over fbm::steady_body;
// docs/design/linearize.md, "Discrete LQR trackers on the device"). Included by fb_capi.hip after fb_dpid.inc (the d verbs' handle check).
// Reference: f_periodic! of LQR, FP/control.jl:708-743, is the law Cessna172Xv2's five trackers and Robot2D's one run every dt = 0.02;
// FA design/c172/c172x_design.jl designs their gains in continuous time (fb_surgery.inc, flightbatch/surgery.py). Here one call steps every
// (system, candidate) pair under the law as it runs; the design chain on top of it is host-side (flightbatch/dtracker.py).
// Every refusal is decided here, before anything is launched.

extern "C" {

int32_t fb_lss_dtracker_metrics(fb_handle h, const int32_t* iz, int32_t nz, const double* K_fbk, const double* K_fwd, const double* K_int,
                                const double* bounds, int32_t m, const double* zref, double t_sim, int32_t stride, double* zmet, double* umet,
                                int32_t* counts, double* zs, double* us, int32_t* status) {
    static const char* verb = "fb_lss_dtracker_metrics";
    if (int32_t rc = dverb_handle(verb, h, FB_DTRACK_ROWS_MAX - 2, "nx + nu + nz <= FB_DTRACK_ROWS_MAX")) return rc;
    const LssState* L = h->lss;
    const int nx = L->nx, nu = L->nu, ny = L->ny;
    if (nu > 8) return fail("%s: nu = %d, a call takes 1 <= nu <= 8 inputs", verb, nu);
    if (nz < 1 || nz > 8) return fail("%s: nz = %d, a call takes 1 <= nz <= 8 command variables", verb, (int)nz);
    if (nx + nu + nz > FB_DTRACK_ROWS_MAX)
        return fail("%s: nx + nu + nz = %d exceeds FB_DTRACK_ROWS_MAX = %d", verb, nx + nu + (int)nz, (int)FB_DTRACK_ROWS_MAX);
    if (!iz) return fail("%s: iz is required", verb);
    if (!lists_in_range(verb, iz, nz, ny, "iz")) return -1;
    if (m < 1 || m > 64) return fail("%s: m = %d, a call takes 1 <= m <= 64 candidates per system", verb, (int)m);
    if (h->n * (int64_t)m > ((int64_t)1 << 31) - 1)
        return fail("%s: %lld systems x %d candidates exceed the 2^31 - 1 pairs of one launch grid", verb, (long long)h->n, (int)m);
    const double Ts = L->Ts;
    if (!std::isfinite(t_sim)) return fail("%s: t_sim = %g must be finite", verb, t_sim);
    const double ticks = std::round(t_sim / Ts);
    if (!(ticks >= 1.0) || !(ticks <= 200000.0))
        return fail("%s: t_sim / Ts = %g ticks (t_sim = %g, Ts = %g), a call takes 1 <= N <= 200000", verb, ticks, t_sim, Ts);
    if (stride < 1) return fail("%s: stride = %d must be at least 1", verb, (int)stride);
    if (!K_fbk || !K_fwd || !K_int || !zref || !status) return fail("%s: K_fbk, K_fwd, K_int, zref and status are required", verb);
    for (int c = 0; c < nz; c++)
        if (!std::isfinite(zref[c])) return fail("%s: zref[%d] = %g must be finite", verb, c, zref[c]);
    const size_t n = (size_t)h->n, nc = n * (size_t)m;
    for (size_t k = 0; bounds && k < (size_t)nu * nc; k++) {
        const double lo = bounds[k], hi = bounds[(size_t)nu * nc + k];
        if (lo != lo || hi != hi || !(lo < hi))
            return fail("%s: bounds lo = %g, hi = %g at system %lld, candidate %lld, input %lld: the output bounds must satisfy lo < hi (either may be infinite)",
                        verb, lo, hi, (long long)(k % n), (long long)((k / n) % (size_t)m), (long long)(k / nc));
    }
    const int N = (int)ticks, ns = fb_lss_stepinfo_samples(N, stride);
    HIPCHK(hipSetDevice(h->device));
    // one device block: K_fbk | K_fwd | K_int | bounds | zref | zmet | umet | zs | us; iz | counts | status apart
    const size_t nfb = (size_t)nu * nx * nc, nfw = (size_t)nu * nz * nc, nb = bounds ? 2 * (size_t)nu * nc : 0;
    const size_t nzm = zmet ? 3 * (size_t)nz * nc : 0, num = umet ? 2 * (size_t)nu * nc : 0, nk = counts ? 2 * (size_t)nu * nc : 0;
    const size_t nzs = zs ? (size_t)ns * nz * nc : 0, nus = us ? (size_t)ns * nu * nc : 0;
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, nfb + 2 * nfw + nb + (size_t)nz + nzm + num + nzs + nus)) return rc;
    if (int32_t rc = blocks.alloc(&di, (size_t)nz + nk + nc)) return rc;
    double *d_fb = d, *d_fw = d_fb + nfb, *d_in = d_fw + nfw, *d_bnd = d_in + nfw, *d_zr = d_bnd + nb, *d_zm = d_zr + nz, *d_um = d_zm + nzm,
           *d_zs = d_um + num, *d_us = d_zs + nzs;
    HIPCHK(hipMemcpyAsync(d_fb, K_fbk, sizeof(double) * nfb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_fw, K_fwd, sizeof(double) * nfw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_in, K_int, sizeof(double) * nfw, hipMemcpyHostToDevice, h->stream));
    if (bounds) HIPCHK(hipMemcpyAsync(d_bnd, bounds, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_zr, zref, sizeof(double) * nz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(di, iz, sizeof(int32_t) * nz, hipMemcpyHostToDevice, h->stream));
    fbj::DTrackArgs a = {};
    verb_args(a, h);
    a.iz = di; a.kfbk = d_fb; a.kfwd = d_fw; a.kint = d_in; a.bounds = bounds ? d_bnd : nullptr; a.zref = d_zr;
    a.zmet = zmet ? d_zm : nullptr; a.umet = umet ? d_um : nullptr; a.counts = counts ? di + nz : nullptr;
    a.zs = zs ? d_zs : nullptr; a.us = us ? d_us : nullptr; a.status = di + nz + nk;
    a.nz = nz; a.m = m; a.nticks = N; a.stride = stride; a.Ts = Ts;
    if (int32_t rc = family_launch(h, group_for(nx + nu + nz), (int64_t)nc, a, [](auto P) { return fbj::k_dtracker<P.value>; })) return rc;
    if (zmet) HIPCHK(hipMemcpyAsync(zmet, d_zm, sizeof(double) * nzm, hipMemcpyDeviceToHost, h->stream));
    if (umet) HIPCHK(hipMemcpyAsync(umet, d_um, sizeof(double) * num, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(hipMemcpyAsync(counts, di + nz, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, h->stream));
    if (zs) HIPCHK(hipMemcpyAsync(zs, d_zs, sizeof(double) * nzs, hipMemcpyDeviceToHost, h->stream));
    if (us) HIPCHK(hipMemcpyAsync(us, d_us, sizeof(double) * nus, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, di + nz + nk, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int32_t fb_lss_dsteady(fb_handle h, const int32_t* iz, int32_t nz, const double* K, const double* K_xi, int32_t k_per_system, double* X, double* U,
                       double* K_fbk, double* K_fwd, double* rpiv, int32_t* status) {
    static const char* verb = "fb_lss_dsteady";
    if (int32_t rc = dverb_handle(verb, h, FB_SURGERY_N_MAX - 1, "nx + nu <= FB_SURGERY_N_MAX")) return rc;
    return steady_run(verb, h, true, iz, nz, K, K_xi, k_per_system, X, U, K_fbk, K_fwd, rpiv, status);
}

}  // extern "C"
