// fb_lqr.inc — lqr(P, Q, R) on a Model(lss) batch (include/flightbatch.h: fb_lqr, fb_lss_get_model; kernels: lqr_kernels.hpp;
// docs/design/linearize.md, "LQR design on the device"). Included by fb_capi.hip after fb_lss.inc.
// Reference: the design scripts call lqr(P, Q, R) on a linearised model at every node of a gain schedule (FA design/c172/c172x_design.jl:181,
// 369, 475, 588, 651; design/robot2d/robot2d_design.jl:58). Q and R are the batch's; A and B are each system's, read where the stepper reads them.

static int lqr_group(int nx) { return 2 * nx <= 8 ? 8 : 2 * nx <= 16 ? 16 : 32; }

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
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("fb_lss_get_model: the handle is not a LinearizedSS handle (fb_lss_create)");
    if (int32_t rc = lss_ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const LssState* L = h->lss;
    const int64_t n = h->n, G = L->G, S = n * G, nx = L->nx, nu = L->nu;
    std::vector<double> ab((size_t)(G + nu) * S);   // the kernels' padded copy, un-padded here
    HIPCHK(hipMemcpyAsync(ab.data(), L->ab, sizeof(double) * ab.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int64_t c = 0; c < nx + nu; c++) {
        double* out = c < nx ? A : B;
        if (!out) continue;
        const int64_t col = c < nx ? c : G + (c - nx), oc = c < nx ? c : c - nx;
        for (int64_t r = 0; r < nx; r++)
            for (int64_t i = 0; i < n; i++) out[(r + nx * oc) * n + i] = ab[col * S + i * G + r];
    }
    return 0;
}

int32_t fb_lqr(fb_handle h, const double* Q, const double* R, double* K, double* X, double* resid, int32_t* iters, int32_t* status) {
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("fb_lqr: the handle is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)");
    const LssState* L = h->lss;
    const int nx = L->nx, nu = L->nu;
    if (nx > FB_LQR_NX_MAX) return fail("fb_lqr: nx = %d, the design takes 1 <= nx <= %d (FB_LQR_NX_MAX)", nx, (int)FB_LQR_NX_MAX);
    if (!L->have_model) return fail("fb_lqr: this LinearizedSS handle has no model yet (fb_lss_set_model)");
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
    double* d = nullptr;
    int32_t* di = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(double) * (nq + nk + nX + nr)));
    auto run = [&]() -> int32_t {
        HIPCHK(hipMalloc(&di, sizeof(int32_t) * 2 * n));
        HIPCHK(hipMemcpyAsync(d, Q, sizeof(double) * nq, hipMemcpyHostToDevice, h->stream));
        a.ab = L->ab; a.q = d;
        a.K = K ? d + nq : nullptr; a.X = X ? d + nq + nk : nullptr; a.resid = resid ? d + nq + nk + nX : nullptr;
        a.iters = di; a.status = di + n;
        a.n = h->n; a.nx = nx; a.nu = nu; a.G = L->G;
        const int P = lqr_group(nx);
        const dim3 grid = grid_for(h->n, fbq::LQR_WAVE / P), block(fbq::LQR_WAVE);
        const bool stamp = h->timing && h->lev_used < h->lev_max;
        if (stamp) HIPCHK(hipEventRecord(h->lev[2 * h->lev_used], h->stream));
        if (P == 8) hipLaunchKernelGGL(fbq::k_lqr<8>, grid, block, 0, h->stream, a);
        else if (P == 16) hipLaunchKernelGGL(fbq::k_lqr<16>, grid, block, 0, h->stream, a);
        else hipLaunchKernelGGL(fbq::k_lqr<32>, grid, block, 0, h->stream, a);
        if (stamp) { HIPCHK(hipEventRecord(h->lev[2 * h->lev_used + 1], h->stream)); h->lev_used++; }
        HIPCHK(hipGetLastError());
        if (K) HIPCHK(hipMemcpyAsync(K, a.K, sizeof(double) * nk, hipMemcpyDeviceToHost, h->stream));
        if (X) HIPCHK(hipMemcpyAsync(X, a.X, sizeof(double) * nX, hipMemcpyDeviceToHost, h->stream));
        if (resid) HIPCHK(hipMemcpyAsync(resid, a.resid, sizeof(double) * nr, hipMemcpyDeviceToHost, h->stream));
        if (iters) HIPCHK(hipMemcpyAsync(iters, a.iters, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
        if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
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
