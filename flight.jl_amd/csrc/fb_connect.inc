// fb_connect.inc — connect / series / feedback on Model(lss) batches (include/flightbatch.h: fb_lss_connect, fb_lss_get_cd; kernels:
// connect_kernels.hpp; docs/design/linearize.md, "Closing loops on the device"). Included by fb_capi.hip after fb_lss.inc (the verbs' shared scaffold).
// Reference: the `connect`, `series` and `feedback` calls between the design verbs of FA design/c172/c172x_design.jl:199-216, 226-227, 244-263,
// 287-292, 317-322, 395-425, 601-617, 724-727, 754-757, and the `connect` cells of design/robot2d/robot2d_design.ipynb.
// Every refusal is decided here, before anything is launched or created. The kernel runs on the plant's stream (where fb_timing_begin_per_launch
// on the plant stamps it); the new handle's copy of the model is then written by k_lss_gather with the identity lists, like every other.

extern "C" {

int32_t fb_lss_get_cd(fb_handle h, double* C, double* D) {
    return lss_unpad("fb_lss_get_cd", h, true, C, D, [](const LssState* L, int64_t n, int64_t i, int r, int c) { return fbg::cd_index(n, i, L->ny, r, c); });
}

int32_t fb_lss_connect(fb_handle p, fb_handle c, const int32_t* jz, int32_t nf, const double* F, int32_t f_per_system,
                       const double* G, int32_t g_per_system, int32_t nw, const int32_t* iz, int32_t ny, int32_t* status, fb_handle* out) {
    if (!out) return fail("fb_lss_connect: out is null");
    *out = nullptr;
    if (!p) return fail("fb_lss_connect: null handle (the plant)");
    if (!is_lss(p)) return fail("fb_lss_connect: the plant is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)");
    if (c && !is_lss(c)) return fail("fb_lss_connect: the compensator is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)");
    if (!p->lss->have_model) return fail("fb_lss_connect: the plant has no model yet (fb_lss_set_model)");
    if (c && !c->lss->have_model) return fail("fb_lss_connect: the compensator has no model yet (fb_lss_set_model)");
    if (int32_t rc = verb_continuous("fb_lss_connect", p)) return rc;
    if (c) { if (int32_t rc = verb_continuous("fb_lss_connect", c)) return rc; }
    if (c && c->device != p->device) return fail("fb_lss_connect: the compensator is on device %d, the plant on device %d", c->device, p->device);
    if (c && c->n != p->n) return fail("fb_lss_connect: the compensator has N = %lld systems, the plant N = %lld", (long long)c->n, (long long)p->n);
    const LssState *Lp = p->lss, *Lc = c ? c->lss : nullptr;
    const int nxp = Lp->nx, nup = Lp->nu, nyp = Lp->ny, nxc = c ? Lc->nx : 0, nuc = c ? Lc->nu : 0, nyc = c ? Lc->ny : 0;
    const int nx = nxp + nxc, nv = nup + nuc, nz = nyp + nyc;
    if (nx > fbl::LSS_NX_MAX) return fail("fb_lss_connect: nx_p + nx_c = %d, the new model takes at most %d states", nx, fbl::LSS_NX_MAX);
    if (nv > FB_CONNECT_NV_MAX) return fail("fb_lss_connect: nv = nu_p + nu_c = %d exceeds FB_CONNECT_NV_MAX = %d", nv, (int)FB_CONNECT_NV_MAX);
    if (nz > FB_CONNECT_NZ_MAX) return fail("fb_lss_connect: nz = ny_p + ny_c = %d exceeds FB_CONNECT_NZ_MAX = %d", nz, (int)FB_CONNECT_NZ_MAX);
    if (nf < 1 || nf > FB_CONNECT_NF_MAX) return fail("fb_lss_connect: nf = %d, the feedback reads 1 <= nf <= %d rows (FB_CONNECT_NF_MAX)", (int)nf, (int)FB_CONNECT_NF_MAX);
    if (nw < 1 || nw > fbl::LSS_NU_MAX) return fail("fb_lss_connect: nw = %d, the new model takes 1 <= nw <= %d inputs", (int)nw, fbl::LSS_NU_MAX);
    if (!F || !G || !jz) return fail("fb_lss_connect: F, G and jz are required");
    if (!iz) {
        if (nz > fbl::LSS_NY_MAX) return fail("fb_lss_connect: iz is NULL (every row of z) and nz = %d exceeds the %d outputs of a LinearizedSS handle", nz, fbl::LSS_NY_MAX);
        ny = nz;
    }
    if (ny < 1 || ny > fbl::LSS_NY_MAX) return fail("fb_lss_connect: ny = %d, the new model takes 1 <= ny <= %d outputs", (int)ny, fbl::LSS_NY_MAX);
    if (!lists_in_range("fb_lss_connect", jz, nf, nz, "jz") || !lists_in_range("fb_lss_connect", iz, ny, nz, "iz")) return -1;

    HIPCHK(hipSetDevice(p->device));
    const int64_t n = p->n;
    const size_t un = (size_t)n;
    const size_t szF = (size_t)nv * nf * (f_per_system ? un : 1), szG = (size_t)nv * nw * (g_per_system ? un : 1);
    const Staged staged(nx, nw, ny, n);
    std::vector<int32_t> idx(jz, jz + nf);
    for (int k = 0; k < ny; k++) idx.push_back(iz ? iz[k] : k);
    NewHandle made;   // (destroyed on every failing path below, after the blocks are freed)
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (c) HIPCHK(hipStreamSynchronize(c->stream));   // (the compensator's model, should its stream still be writing it)
    if (int32_t rc = blocks.alloc(&d, szF + szG + staged.doubles)) return rc;
    if (int32_t rc = blocks.alloc(&di, idx.size() + un)) return rc;
    if (int32_t rc = lss_new_handle(nx, nw, ny, n, p->device, &made.h)) return rc;
    double *dF = d, *dG = dF + szF, *dS = dG + szG;
    HIPCHK(hipMemcpyAsync(dF, F, sizeof(double) * szF, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(dG, G, sizeof(double) * szG, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(di, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemsetAsync(dS, 0, sizeof(double) * staged.AB, p->stream));   // deviation coordinates: xdot0, x0, u0, y0 are zero
    fbc::ConnectArgs a = {};
    a.p = {Lp->ab, Lp->cd, nxp, nup, nyp, Lp->G};
    if (c) a.c = {Lc->ab, Lc->cd, nxc, nuc, nyc, Lc->G};
    a.jz = di; a.iz = di + nf;
    a.F = dF; a.f_e = f_per_system ? n : 1; a.f_s = f_per_system ? 1 : 0;
    a.G = dG; a.g_e = g_per_system ? n : 1; a.g_s = g_per_system ? 1 : 0;
    a.AB = dS + staged.AB; a.CD = dS + staged.CD; a.status = di + idx.size();
    a.n = n; a.nf = nf; a.nw = nw; a.ny = ny;
    if (int32_t rc = family_launch(p, group_for(nx > nv ? nx : nv), n, a, [](auto P) { return fbc::k_connect<P.value>; })) return rc;
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * un, hipMemcpyDeviceToHost, p->stream));
    return lss_adopt(p, made, staged.src(dS), nullptr, nullptr, nullptr, out);
}

}  // extern "C"
