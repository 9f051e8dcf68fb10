// fb_c2d.inc — zero-order-hold discretisation of Model(lss) batches (include/flightbatch.h: fb_lss_c2d, fb_lss_sample_time; kernel:
// c2d_kernels.hpp; docs/design/linearize.md, "Sampled models on the device"). Included by fb_capi.hip after fb_surgery.inc.
// Reference: ControlSystems' step and lsim discretise exactly before they simulate (FA design/pidopt.jl: step(T, t_sim);
// demos/c172_demos.jl: lsim(e2q, ...)); here the sampled model is a handle of its own, which fb_step and fb_lss_stepinfo then run.
// Every refusal is decided here, before anything is launched or created. The kernel runs on the source's stream (where
// fb_timing_begin_per_launch on the source stamps it); the new handle's copy of the model is then written by k_lss_gather, like
// fb_lss_transform's.

extern "C" {

int32_t fb_lss_c2d(fb_handle src, double Ts, int32_t* squarings, int32_t* status, fb_handle* out) {
    static const char* verb = "fb_lss_c2d";
    if (!out) return fail("fb_lss_c2d: out is null");
    *out = nullptr;
    if (int32_t rc = verb_handle(verb, src, fbl::LSS_NX_MAX, "discretisation", "a LinearizedSS handle's")) return rc;
    if (int32_t rc = verb_model(verb, src)) return rc;
    const LssState* L = src->lss;
    if (L->Ts > 0.0) return fail("fb_lss_c2d: the handle is itself a sampled model (Ts = %g): discretise the continuous model it was made from", L->Ts);
    if (!(Ts > 0.0) || !std::isfinite(Ts)) return fail("fb_lss_c2d: Ts = %g must be positive and finite", Ts);
    const int nx = L->nx, nu = L->nu, ny = L->ny;

    HIPCHK(hipSetDevice(src->device));
    const int64_t n = src->n;
    const size_t un = (size_t)n;
    const Staged staged(nx, nu, ny, n);
    NewHandle made;   // (destroyed on every failing path below, after the blocks are freed)
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, staged.doubles)) return rc;
    if (int32_t rc = blocks.alloc(&di, 2 * un)) return rc;
    if (int32_t rc = lss_new_handle(nx, nu, ny, n, src->device, &made.h)) return rc;
    fbz::C2dArgs a = {};
    verb_args(a, src);
    a.xs = L->xs; a.u0 = L->u0; a.y0 = L->y0;
    a.Ts = Ts;
    a.xdot0 = d; a.x0 = d + staged.x0; a.u0_out = d + staged.u0; a.y0_out = d + staged.y0;
    a.AB = d + staged.AB; a.CD = d + staged.CD;
    a.squarings = di; a.status = di + un;
    if (int32_t rc = family_launch(src, group_for(nx), n, a, [](auto P) { return fbz::k_lss_c2d<P.value>; })) return rc;
    if (squarings) HIPCHK(hipMemcpyAsync(squarings, a.squarings, sizeof(int32_t) * un, hipMemcpyDeviceToHost, src->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * un, hipMemcpyDeviceToHost, src->stream));
    fb_handle h = nullptr;
    if (int32_t rc = lss_adopt(src, made, staged.src(d), nullptr, nullptr, nullptr, &h)) return rc;
    h->lss->Ts = Ts;          // sampled: fb_step runs the map, the clock advances by Ts
    h->params.dt = Ts;
    *out = h;
    return 0;
}

int32_t fb_lss_sample_time(fb_handle h, double* Ts) {
    if (!h) return fail("fb_lss_sample_time: null handle");
    if (!is_lss(h)) return fail("fb_lss_sample_time: the handle is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)");
    if (!Ts) return fail("fb_lss_sample_time: Ts is null");
    *Ts = h->lss ? h->lss->Ts : 0.0;
    return 0;
}

}  // extern "C"
