// fb_dlqr.inc — the discrete LQR of sampled Model(lss) batches (include/flightbatch.h: fb_lss_dlqr; kernel: dlqr_kernels.hpp;
// docs/design/linearize.md, "Discrete LQR on the device"). Included by fb_capi.hip after fb_c2d.inc.
// Reference: ControlSystems' lqr(Discrete, Phi, Gamma, Q, R); the controllers of FP/control.jl (LQR, PID, Integrator) run in f_periodic!
// at dt = 0.02 with gains the design scripts computed in continuous time. Q and R are the batch's, checked as fb_lqr checks them
// (fb_lqr.inc: lqr_symmetric, lqr_rinv); Phi and Gamma are each system's, read where k_lss_map reads them.
// Every refusal is decided here, before anything is launched or created. The kernel runs on the source's stream (where
// fb_timing_begin_per_launch on the source stamps it); the closed handle's copy of the model is then written by k_lss_gather, like fb_lss_c2d's.

extern "C" {

int32_t fb_lss_dlqr(fb_handle src, const double* Q, const double* R, double* K, double* X, double* resid, int32_t* iters, int32_t* status,
                    fb_handle* closed) {
    static const char* verb = "fb_lss_dlqr";
    if (closed) *closed = nullptr;
    if (int32_t rc = verb_handle(verb, src, FB_DLQR_NX_MAX, "discrete design", "FB_DLQR_NX_MAX")) return rc;
    if (int32_t rc = verb_model(verb, src)) return rc;
    const LssState* L = src->lss;
    if (!(L->Ts > 0.0)) return fail("fb_lss_dlqr: a discrete-time verb on a continuous model: sample it first (fb_lss_c2d makes the sampled handle this verb designs on)");
    const int nx = L->nx, nu = L->nu, ny = L->ny;
    if (!Q || !R) return fail("fb_lss_dlqr: Q and R are required");
    if (!lqr_symmetric(Q, nx)) return fail("fb_lss_dlqr: Q is not symmetric");
    if (!lqr_symmetric(R, nu)) return fail("fb_lss_dlqr: R is not symmetric");
    static_assert(fbk::DLQR_NU_MAX == fbq::LQR_NU_MAX && fbk::DLQR_NU_MAX == fbl::LSS_NU_MAX, "lqr_rinv's inverse fills DlqrArgs::rinv");
    fbk::DlqrArgs a = {};
    if (!lqr_rinv(R, nu, a.rinv)) return fail("fb_lss_dlqr: R is not positive definite");
    for (int k = 0; k < nx * nx; k++) {
        if (!std::isfinite(Q[k])) return fail("fb_lss_dlqr: Q has a non-finite entry");
        a.qmax = std::fmax(a.qmax, std::fabs(Q[k]));
    }
    HIPCHK(hipSetDevice(src->device));
    const int64_t n = src->n;
    const size_t un = (size_t)n;
    // one device block: Q | K | X | resid | the closed model's staging; iters, status
    const Staged staged(nx, nu, ny, n);
    const size_t nq = (size_t)nx * nx, nk = K ? (size_t)nu * nx * un : 0, nX = X ? nq * un : 0, nr = resid ? un : 0;
    NewHandle made;   // (destroyed on every failing path below, after the blocks are freed)
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, nq + nk + nX + nr + (closed ? staged.doubles : 0))) return rc;
    if (int32_t rc = blocks.alloc(&di, 2 * un)) return rc;
    if (closed) {
        if (int32_t rc = lss_new_handle(nx, nu, ny, n, src->device, &made.h)) return rc;
    }
    HIPCHK(hipMemcpyAsync(d, Q, sizeof(double) * nq, hipMemcpyHostToDevice, src->stream));
    verb_args(a, src);
    a.xs = L->xs; a.u0 = L->u0; a.y0 = L->y0;
    a.q = d;
    a.K = K ? d + nq : nullptr; a.X = X ? d + nq + nk : nullptr; a.resid = resid ? d + nq + nk + nX : nullptr;
    a.iters = di; a.status = di + un;
    double* m = d + nq + nk + nX + nr;
    if (closed) {
        a.xdot0 = m; a.x0 = m + staged.x0; a.u0_out = m + staged.u0; a.y0_out = m + staged.y0;
        a.AB = m + staged.AB; a.CD = m + staged.CD;
    }
    // (nx <= FB_DLQR_NX_MAX: the 32-lane instance does not exist)
    if (int32_t rc = family_launch(src, group_for(nx), n, a, [](auto P) {
            if constexpr (P.value <= FB_DLQR_NX_MAX) return fbk::k_lss_dlqr<P.value>;
            else return static_cast<void (*)(fbk::DlqrArgs)>(nullptr);
        })) return rc;
    if (K) HIPCHK(hipMemcpyAsync(K, a.K, sizeof(double) * nk, hipMemcpyDeviceToHost, src->stream));
    if (X) HIPCHK(hipMemcpyAsync(X, a.X, sizeof(double) * nX, hipMemcpyDeviceToHost, src->stream));
    if (resid) HIPCHK(hipMemcpyAsync(resid, a.resid, sizeof(double) * nr, hipMemcpyDeviceToHost, src->stream));
    if (iters) HIPCHK(hipMemcpyAsync(iters, a.iters, sizeof(int32_t) * un, hipMemcpyDeviceToHost, src->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * un, hipMemcpyDeviceToHost, src->stream));
    if (!closed) {
        HIPCHK(hipStreamSynchronize(src->stream));
        return 0;
    }
    fb_handle h = nullptr;
    if (int32_t rc = lss_adopt(src, made, staged.src(m), nullptr, nullptr, nullptr, &h)) return rc;
    h->lss->Ts = L->Ts;       // sampled, as its source: fb_step runs the map, the clock advances by Ts
    h->params.dt = L->Ts;
    *closed = h;
    return 0;
}

}  // extern "C"
