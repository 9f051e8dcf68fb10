// fb_poles.inc — the poles of a Model(lss) batch (include/flightbatch.h: fb_lss_poles; kernels: poles_kernels.hpp;
// docs/design/linearize.md, "Poles on the device"). Included by fb_capi.hip after fb_lss.inc (the verbs' shared scaffold).
// Reference: FA design/robot2d/robot2d_design.ipynb calls dampreport(P) on the linearised vehicle and on the LQR velocity loop; here one call
// finds the poles of every system of a batch, and flightbatch/poles.py derives dampreport's columns from them.

extern "C" {

int32_t fb_lss_poles(fb_handle h, double* re, double* im, int32_t* iters, int32_t* status) {
    if (int32_t rc = verb_handle("fb_lss_poles", h, FB_POLES_NX_MAX, "call", "FB_POLES_NX_MAX")) return rc;
    if (int32_t rc = verb_model("fb_lss_poles", h)) return rc;
    if (int32_t rc = verb_continuous("fb_lss_poles", h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->n, np = (size_t)h->lss->nx * n;
    // one device block: re | im; iters, status apart
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
