// fb_dconnect.inc — connect on SAMPLED Model(lss) batches, with unit delays (include/flightbatch.h: fb_lss_dconnect; kernels:
// dconnect_kernels.hpp; docs/design/linearize.md, "Closing sampled loops on the device"). Included by fb_capi.hip after fb_connect.inc.
// Reference: the `connect`, `series` and `feedback` calls of FA design/c172/c172x_design.jl on the loops that FP/control.jl then runs in
// f_periodic! every dt = 0.02; the unit delay is the sample of computational delay between a controller's read and its write.
// fb_lss_connect's host side with a list more: every refusal is decided here, before anything is launched or created. The kernel runs on the
// plant's stream; the new handle's copy of the model is written by k_lss_gather with the identity lists and is then marked sampled.

extern "C" {

int32_t fb_lss_dconnect(fb_handle p, fb_handle c, const int32_t* dz, int32_t nd, const int32_t* jz, int32_t nf, const double* F, int32_t f_per_system,
                        const double* G, int32_t g_per_system, int32_t nw, const int32_t* iz, int32_t ny, int32_t* status, fb_handle* out) {
    static const char* verb = "fb_lss_dconnect";
    if (!out) return fail("%s: out is null", verb);
    *out = nullptr;
    if (!p) return fail("%s: null handle (the plant)", verb);
    if (!is_lss(p)) return fail("%s: the plant is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)", verb);
    if (c && !is_lss(c)) return fail("%s: the compensator is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)", verb);
    if (!p->lss->have_model) return fail("%s: the plant has no model yet (fb_lss_set_model)", verb);
    if (c && !c->lss->have_model) return fail("%s: the compensator has no model yet (fb_lss_set_model)", verb);
    if (!(p->lss->Ts > 0.0))
        return fail("%s: a discrete-time verb on a continuous model: the plant is not sampled (fb_lss_c2d, or fb_lss_set_sampled on a model that holds Phi and Gamma)", verb);
    if (c && !(c->lss->Ts > 0.0))
        return fail("%s: a discrete-time verb on a continuous model: the compensator is not sampled (fb_lss_c2d, or fb_lss_set_sampled on a model that holds Phi and Gamma)", verb);
    if (c && memcmp(&c->lss->Ts, &p->lss->Ts, sizeof(double)) != 0)
        return fail("%s: the compensator's Ts = %.17g differs from the plant's Ts = %.17g (one sample time for the whole loop)", verb, c->lss->Ts, p->lss->Ts);
    if (c && c->device != p->device) return fail("%s: the compensator is on device %d, the plant on device %d", verb, c->device, p->device);
    if (c && c->n != p->n) return fail("%s: the compensator has N = %lld systems, the plant N = %lld", verb, (long long)c->n, (long long)p->n);
    const LssState *Lp = p->lss, *Lc = c ? c->lss : nullptr;
    const int nxp = Lp->nx, nup = Lp->nu, nyp = Lp->ny, nxc = c ? Lc->nx : 0, nuc = c ? Lc->nu : 0, nyc = c ? Lc->ny : 0;
    const int nx = nxp + nxc, nv = nup + nuc, nz = nyp + nyc;
    if (nd < 0 || nd > FB_DCONNECT_ND_MAX) return fail("%s: nd = %d, a call delays 0 <= nd <= %d rows (FB_DCONNECT_ND_MAX)", verb, (int)nd, (int)FB_DCONNECT_ND_MAX);
    if (nd > 0 && !dz) return fail("%s: nd = %d and dz is NULL", verb, (int)nd);
    const int nxe = nx + nd, nze = nz + nd;
    if (nxe > fbl::LSS_NX_MAX) return fail("%s: nx_p + nx_c + nd = %d, the new model takes at most %d states", verb, nxe, fbl::LSS_NX_MAX);
    if (nv > FB_CONNECT_NV_MAX) return fail("%s: nv = nu_p + nu_c = %d exceeds FB_CONNECT_NV_MAX = %d", verb, nv, (int)FB_CONNECT_NV_MAX);
    if (nze > FB_CONNECT_NZ_MAX) return fail("%s: nz + nd = ny_p + ny_c + nd = %d exceeds FB_CONNECT_NZ_MAX = %d", verb, nze, (int)FB_CONNECT_NZ_MAX);
    if (nf < 1 || nf > FB_CONNECT_NF_MAX) return fail("%s: nf = %d, the feedback reads 1 <= nf <= %d rows (FB_CONNECT_NF_MAX)", verb, (int)nf, (int)FB_CONNECT_NF_MAX);
    if (nw < 1 || nw > fbl::LSS_NU_MAX) return fail("%s: nw = %d, the new model takes 1 <= nw <= %d inputs", verb, (int)nw, fbl::LSS_NU_MAX);
    if (!F || !G || !jz) return fail("%s: F, G and jz are required", verb);
    if (!iz) {
        if (nze > fbl::LSS_NY_MAX) return fail("%s: iz is NULL (every row of [z; q]) and nz + nd = %d exceeds the %d outputs of a LinearizedSS handle", verb, nze, fbl::LSS_NY_MAX);
        ny = nze;
    }
    if (ny < 1 || ny > fbl::LSS_NY_MAX) return fail("%s: ny = %d, the new model takes 1 <= ny <= %d outputs", verb, (int)ny, fbl::LSS_NY_MAX);
    if (!lists_in_range(verb, dz, nd, nz, "dz") || !lists_in_range(verb, jz, nf, nze, "jz") || !lists_in_range(verb, iz, ny, nze, "iz")) return -1;

    HIPCHK(hipSetDevice(p->device));
    const int64_t n = p->n;
    const size_t un = (size_t)n;
    const size_t szF = (size_t)nv * nf * (f_per_system ? un : 1), szG = (size_t)nv * nw * (g_per_system ? un : 1);
    const Staged staged(nxe, nw, ny, n);
    std::vector<int32_t> idx(jz, jz + nf);
    for (int k = 0; k < ny; k++) idx.push_back(iz ? iz[k] : k);
    for (int k = 0; k < nd; k++) idx.push_back(dz[k]);
    NewHandle made;   // (destroyed on every failing path below, after the blocks are freed)
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (c) HIPCHK(hipStreamSynchronize(c->stream));   // (the compensator's model, should its stream still be writing it)
    if (int32_t rc = blocks.alloc(&d, szF + szG + staged.doubles)) return rc;
    if (int32_t rc = blocks.alloc(&di, idx.size() + un)) return rc;
    if (int32_t rc = lss_new_handle(nxe, nw, ny, n, p->device, &made.h)) return rc;
    double *dF = d, *dG = dF + szF, *dS = dG + szG;
    HIPCHK(hipMemcpyAsync(dF, F, sizeof(double) * szF, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(dG, G, sizeof(double) * szG, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(di, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemsetAsync(dS, 0, sizeof(double) * staged.AB, p->stream));   // deviation coordinates: delta, x0, u0, y0 are zero
    fbv::DConnectArgs a = {};
    a.p = {Lp->ab, Lp->cd, nxp, nup, nyp, Lp->G};
    if (c) a.c = {Lc->ab, Lc->cd, nxc, nuc, nyc, Lc->G};
    a.jz = di; a.iz = di + nf; a.dz = di + nf + ny;
    a.F = dF; a.f_e = f_per_system ? n : 1; a.f_s = f_per_system ? 1 : 0;
    a.G = dG; a.g_e = g_per_system ? n : 1; a.g_s = g_per_system ? 1 : 0;
    a.AB = dS + staged.AB; a.CD = dS + staged.CD; a.status = di + idx.size();
    a.n = n; a.nf = nf; a.nw = nw; a.ny = ny; a.nd = nd;
    if (int32_t rc = family_launch(p, group_for(nxe > nv ? nxe : nv), n, a, [](auto P) { return fbv::k_dconnect<P.value>; })) return rc;
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * un, hipMemcpyDeviceToHost, p->stream));
    fb_handle h = nullptr;
    if (int32_t rc = lss_adopt(p, made, staged.src(dS), nullptr, nullptr, nullptr, &h)) return rc;
    h->lss->Ts = Lp->Ts;      // sampled, as its sources: fb_step runs the map, the clock advances by Ts
    h->params.dt = Lp->Ts;
    *out = h;
    return 0;
}

}  // extern "C"
