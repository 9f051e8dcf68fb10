// fb_poles.inc — the poles of a Model(lss) batch (include/flightbatch.h: fb_lss_poles; kernels: poles_kernels.hpp;
// docs/design/linearize.md, "Poles on the device"). Included by fb_capi.hip after fb_pid.inc.
// Reference: FA design/robot2d/robot2d_design.ipynb calls dampreport(P) on the linearised vehicle and on the LQR velocity loop; here one call
// finds the poles of every system of a batch, and flightbatch/poles.py derives dampreport's columns from them.

static int poles_group(int nx) { return nx <= 8 ? 8 : nx <= 16 ? 16 : 32; }

extern "C" {

int32_t fb_lss_poles(fb_handle h, double* re, double* im, int32_t* iters, int32_t* status) {
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("fb_lss_poles: the handle is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)");
    const LssState* L = h->lss;
    if (!L) return fail("fb_lss_poles: the handle is not ready (its creation did not finish)");
    const int nx = L->nx;
    if (nx < 1 || nx > FB_POLES_NX_MAX) return fail("fb_lss_poles: nx = %d, the call takes 1 <= nx <= %d (FB_POLES_NX_MAX)", nx, (int)FB_POLES_NX_MAX);
    if (!L->have_model) return fail("fb_lss_poles: this LinearizedSS handle has no model yet (fb_lss_set_model)");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = (size_t)nx * n;
    // one device block: re | im; iters, status apart
    double* d = nullptr;
    int32_t* di = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(double) * 2 * np));
    auto run = [&]() -> int32_t {
        HIPCHK(hipMalloc(&di, sizeof(int32_t) * 2 * n));
        fbe::PolesArgs a = {};
        a.ab = L->ab; a.re = d; a.im = d + np; a.iters = di; a.status = di + n;
        a.n = h->n; a.nx = nx; a.G = L->G;
        const int P = poles_group(nx);
        const dim3 grid = grid_for(h->n, fbe::POLES_WAVE / P), block(fbe::POLES_WAVE);
        const bool stamp = h->timing && h->lev_used < h->lev_max;
        if (stamp) HIPCHK(hipEventRecord(h->lev[2 * h->lev_used], h->stream));
        if (P == 8) hipLaunchKernelGGL(fbe::k_poles<8>, grid, block, 0, h->stream, a);
        else if (P == 16) hipLaunchKernelGGL(fbe::k_poles<16>, grid, block, 0, h->stream, a);
        else hipLaunchKernelGGL(fbe::k_poles<32>, grid, block, 0, h->stream, a);
        if (stamp) { HIPCHK(hipEventRecord(h->lev[2 * h->lev_used + 1], h->stream)); h->lev_used++; }
        HIPCHK(hipGetLastError());
        if (re) HIPCHK(hipMemcpyAsync(re, a.re, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
        if (im) HIPCHK(hipMemcpyAsync(im, a.im, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
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
