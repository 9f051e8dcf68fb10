// fb_lqr.inc — lqr(P, Q, R) on a Model(lss) batch (include/flightbatch.h: fb_lqr, fb_lss_get_model; kernels: lqr_kernels.hpp;
// docs/design/linearize.md, "LQR design on the device"). Included by fb_capi.hip after fb_lss.inc, whose first part is the scaffold every verb here uses.
// Reference: the design scripts call lqr(P, Q, R) on a linearised model at every node of a gain schedule (FA design/c172/c172x_design.jl:181,
// 369, 475, 588, 651; design/robot2d/robot2d_design.jl:58). Q and R are the batch's; A and B are each system's, read where the stepper reads them.

// inv(R) by Cholesky (R = L L', column-major nu x nu); false when R is not positive definite
static bool lqr_rinv(const double* R, int nu, double* rinv) {
    double L[fbq::LQR_NU_MAX][fbq::LQR_NU_MAX] = {}, Li[fbq::LQR_NU_MAX][fbq::LQR_NU_MAX] = {};
    for (int j = 0; j < nu; j++) {
        double d = R[j + nu * j];
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < nu; i++) {
            double s = R[i + nu * j];
            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    for (int j = 0; j < nu; j++) {          // inv(L), lower triangular
        Li[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < nu; i++) {
            double s = 0.0;
            for (int k = j; k < i; k++) s -= L[i][k] * Li[k][j];
            Li[i][j] = s / L[i][i];
        }
    }
    for (int a = 0; a < nu; a++)            // inv(R) = inv(L)' inv(L)
        for (int b = 0; b < nu; b++) {
            double s = 0.0;
            for (int k = (a > b ? a : b); k < nu; k++) s += Li[k][a] * Li[k][b];
            rinv[a * nu + b] = s;
        }
    for (int a = 0; a < nu * nu; a++)
        if (!std::isfinite(rinv[a])) return false;
    return true;
}
static bool lqr_symmetric(const double* M, int n) {
    for (int r = 0; r < n; r++)
        for (int c = 0; c < r; c++)
            if (!(M[r + n * c] == M[c + n * r])) return false;
    return true;
}

extern "C" {

int32_t fb_lss_get_model(fb_handle h, double* A, double* B) {
    return lss_unpad("fb_lss_get_model", h, false, A, B, [](const LssState* L, int64_t n, int64_t i, int r, int c) {
        return fbg::ab_index(n * L->G, i * L->G, c < L->nx ? c : L->G + c - L->nx) + r; });
}

int32_t fb_lqr(fb_handle h, const double* Q, const double* R, double* K, double* X, double* resid, int32_t* iters, int32_t* status) {
    if (int32_t rc = verb_handle("fb_lqr", h, FB_LQR_NX_MAX, "design", "FB_LQR_NX_MAX")) return rc;
    if (int32_t rc = verb_model("fb_lqr", h)) return rc;
    if (int32_t rc = verb_continuous("fb_lqr", h)) return rc;
    const int nx = h->lss->nx, nu = h->lss->nu;
    if (!Q || !R) return fail("fb_lqr: Q and R are required");
    if (!lqr_symmetric(Q, nx)) return fail("fb_lqr: Q is not symmetric");
    if (!lqr_symmetric(R, nu)) return fail("fb_lqr: R is not symmetric");
    fbq::LqrArgs a = {};
    if (!lqr_rinv(R, nu, a.rinv)) return fail("fb_lqr: R is not positive definite");
    for (int k = 0; k < nx * nx; k++) {
        if (!std::isfinite(Q[k])) return fail("fb_lqr: Q has a non-finite entry");
        a.qmax = std::fmax(a.qmax, std::fabs(Q[k]));
    }
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n;
    // one device block: Q | K | X | resid | iters, status
    const size_t nq = (size_t)nx * nx, nk = K ? (size_t)nu * nx * n : 0, nX = X ? nq * n : 0, nr = resid ? n : 0;
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, nq + nk + nX + nr)) return rc;
    if (int32_t rc = blocks.alloc(&di, 2 * n)) return rc;
    HIPCHK(hipMemcpyAsync(d, Q, sizeof(double) * nq, hipMemcpyHostToDevice, h->stream));
    verb_args_ab(a, h);
    a.nu = nu; a.q = d;
    a.K = K ? d + nq : nullptr; a.X = X ? d + nq + nk : nullptr; a.resid = resid ? d + nq + nk + nX : nullptr;
    a.iters = di; a.status = di + n;
    if (int32_t rc = family_launch(h, group_for(2 * nx), h->n, a, [](auto P) { return fbq::k_lqr<P.value>; })) return rc;
    if (K) HIPCHK(hipMemcpyAsync(K, a.K, sizeof(double) * nk, hipMemcpyDeviceToHost, h->stream));
    if (X) HIPCHK(hipMemcpyAsync(X, a.X, sizeof(double) * nX, hipMemcpyDeviceToHost, h->stream));
    if (resid) HIPCHK(hipMemcpyAsync(resid, a.resid, sizeof(double) * nr, hipMemcpyDeviceToHost, h->stream));
    if (iters) HIPCHK(hipMemcpyAsync(iters, a.iters, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
