// fb_surgery.inc — design-model surgery on Model(lss) batches (include/flightbatch.h: fb_lss_transform, fb_lss_steady; kernels:
// surgery_kernels.hpp; docs/design/linearize.md, "Design-model surgery on the device"). Included by fb_capi.hip after fb_connect.inc.
// Reference: get_design_model!, subsystem and delete_vars (FA design/c172/c172x_design.jl:23-82, 144) and K_fwd = M22 + K M12 with
// M = inv([A B; C D]) (:184-188, :371-381, :477-487, :656-665).
// Every refusal is decided here, before anything is launched or created. The kernels run on the source's stream (where
// fb_timing_begin_per_launch on the source stamps them); the new handle's copy of the model is then written by k_lss_gather through the
// subsystem lists, like fb_lss_from_linearization's.

// fb_lss_steady and fb_lss_dsteady (fb_dtracker.inc) behind their handle checks: the sizes, the lists, the blocks and the one kernel, whose
// DISC instance subtracts the identity from Phi while it stages L. K_xi and K_fbk are the discrete verb's only.
static int32_t steady_run(const char* verb, fb_handle h, bool disc, const int32_t* iz, int32_t nz, const double* K, const double* K_xi,
                          int32_t k_per_system, double* X, double* U, double* K_fbk, double* K_fwd, double* rpiv, int32_t* status) {
    const LssState* L = h->lss;
    const int nx = L->nx, nu = L->nu, ny = L->ny;
    if (nx + nu > FB_SURGERY_N_MAX) return fail("%s: nx + nu = %d exceeds FB_SURGERY_N_MAX = %d", verb, nx + nu, (int)FB_SURGERY_N_MAX);
    if (nz != nu) return fail("%s: nz = %d, the map takes as many output rows as the model has inputs (nu = %d)", verb, (int)nz, nu);
    if (!iz) return fail("%s: iz is required", verb);
    if (!lists_in_range(verb, iz, nz, ny, "iz")) return -1;
    if (K_fwd && !K) return fail("%s: K_fwd = U + K X needs K", verb);
    if ((K_xi || K_fbk) && !K) return fail("%s: K_fbk = K - Ts K_xi C_z needs K", verb);

    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->n;
    const size_t un = (size_t)n, per = k_per_system ? un : 1;
    const size_t szK = K ? (size_t)nu * nx * per : 0, szXi = K_xi ? (size_t)nu * nu * per : 0, szX = (size_t)nx * nu * un, szU = (size_t)nu * nu * un;
    const size_t szF = K_fbk ? (size_t)nu * nx * un : 0;
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, szK + szXi + szX + 2 * szU + szF + un)) return rc;
    if (int32_t rc = blocks.alloc(&di, (size_t)nz + un)) return rc;
    fbm::SteadyArgs a = {};
    verb_args(a, h);
    double *dK = d, *dXi = dK + szK;
    a.X = dXi + szXi; a.U = a.X + szX; a.Kfwd = K ? a.U + szU : nullptr; a.Kfbk = K_fbk ? a.U + 2 * szU : nullptr; a.rpiv = a.U + 2 * szU + szF;
    a.iz = di; a.status = di + nz;
    a.Ts = L->Ts;
    HIPCHK(hipMemcpyAsync(di, iz, sizeof(int32_t) * nz, hipMemcpyHostToDevice, h->stream));
    if (K) {
        HIPCHK(hipMemcpyAsync(dK, K, sizeof(double) * szK, hipMemcpyHostToDevice, h->stream));
        a.K = dK; a.k_e = k_per_system ? n : 1; a.k_s = k_per_system ? 1 : 0;
    }
    if (K_xi) {
        HIPCHK(hipMemcpyAsync(dXi, K_xi, sizeof(double) * szXi, hipMemcpyHostToDevice, h->stream));
        a.Kxi = dXi;
    }
    if (disc) {
        if (int32_t rc = family_launch(h, group_for(nx + nu), n, a, [](auto P) { return fbj::k_dsteady<P.value>; })) return rc;
    } else if (int32_t rc = family_launch(h, group_for(nx + nu), n, a, [](auto P) { return fbm::k_steady<P.value>; })) return rc;
    if (X) HIPCHK(hipMemcpyAsync(X, a.X, sizeof(double) * szX, hipMemcpyDeviceToHost, h->stream));
    if (U) HIPCHK(hipMemcpyAsync(U, a.U, sizeof(double) * szU, hipMemcpyDeviceToHost, h->stream));
    if (K_fbk) HIPCHK(hipMemcpyAsync(K_fbk, a.Kfbk, sizeof(double) * szF, hipMemcpyDeviceToHost, h->stream));
    if (K_fwd) HIPCHK(hipMemcpyAsync(K_fwd, a.Kfwd, sizeof(double) * szU, hipMemcpyDeviceToHost, h->stream));
    if (rpiv) HIPCHK(hipMemcpyAsync(rpiv, a.rpiv, sizeof(double) * un, hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * un, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" {

int32_t fb_lss_transform(fb_handle src, const int32_t* rows, const int32_t* xdot_zero, const int32_t* ix, int32_t nxo, const int32_t* iu, int32_t nuo,
                         const int32_t* iy, int32_t nyo, int32_t* status, double* rpiv, fb_handle* out) {
    static const char* verb = "fb_lss_transform";
    if (!out) return fail("fb_lss_transform: out is null");
    *out = nullptr;
    if (int32_t rc = verb_handle(verb, src, fbl::LSS_NX_MAX, "transform", "a LinearizedSS handle's")) return rc;
    if (int32_t rc = verb_model(verb, src)) return rc;
    if (int32_t rc = verb_continuous(verb, src)) return rc;
    const LssState* L = src->lss;
    const int nx = L->nx, nu = L->nu, ny = L->ny;
    if (!ix) nxo = nx;
    if (!iu) nuo = nu;
    if (!iy) nyo = ny;
    if (nxo < 1 || nxo > nx) return fail("fb_lss_transform: nxo = %d, the new model takes 1 <= nxo <= %d of the source's states", (int)nxo, nx);
    if (nuo < 1 || nuo > nu) return fail("fb_lss_transform: nuo = %d, the new model takes 1 <= nuo <= %d of the source's inputs", (int)nuo, nu);
    if (nyo < 1 || nyo > ny) return fail("fb_lss_transform: nyo = %d, the new model takes 1 <= nyo <= %d of the source's outputs", (int)nyo, ny);
    if (!lists_in_range(verb, rows, nx, ny, "rows") || !lists_in_range(verb, ix, nxo, nx, "ix") || !lists_in_range(verb, iu, nuo, nu, "iu") ||
        !lists_in_range(verb, iy, nyo, ny, "iy")) return -1;

    HIPCHK(hipSetDevice(src->device));
    const int64_t n = src->n;
    const size_t un = (size_t)n;
    const Staged staged(nx, nu, ny, n);
    NewHandle made;   // (destroyed on every failing path below, after the blocks are freed)
    DevBlocks blocks;
    double* d = nullptr;
    int32_t* di = nullptr;
    if (int32_t rc = blocks.alloc(&d, staged.doubles + un)) return rc;
    if (int32_t rc = blocks.alloc(&di, (size_t)nx + un)) return rc;
    if (int32_t rc = lss_new_handle(nxo, nuo, nyo, n, src->device, &made.h)) return rc;
    fbm::TransformArgs a = {};
    verb_args(a, src);
    a.xs = L->xs; a.u0 = L->u0; a.y0 = L->y0;
    a.xdot0 = d; a.x0 = d + staged.x0; a.u0_out = d + staged.u0; a.y0_out = d + staged.y0;
    a.AB = d + staged.AB; a.CD = d + staged.CD; a.rpiv = d + staged.doubles;
    a.status = di + nx;
    if (rows) {
        HIPCHK(hipMemcpyAsync(di, rows, sizeof(int32_t) * nx, hipMemcpyHostToDevice, src->stream));
        a.rows = di;
    }
    for (int k = 0; xdot_zero && k < nx; k++)
        if (xdot_zero[k]) a.zero |= 1u << k;
    if (int32_t rc = family_launch(src, group_for(nx), n, a, [](auto P) { return fbm::k_transform<P.value>; })) return rc;
    if (status) HIPCHK(hipMemcpyAsync(status, a.status, sizeof(int32_t) * un, hipMemcpyDeviceToHost, src->stream));
    if (rpiv) HIPCHK(hipMemcpyAsync(rpiv, a.rpiv, sizeof(double) * un, hipMemcpyDeviceToHost, src->stream));
    return lss_adopt(src, made, staged.src(d), ix, iu, iy, out);
}

int32_t fb_lss_steady(fb_handle h, const int32_t* iz, int32_t nz, const double* K, int32_t k_per_system, double* X, double* U, double* K_fwd,
                      double* rpiv, int32_t* status) {
    static const char* verb = "fb_lss_steady";
    if (int32_t rc = verb_handle(verb, h, FB_SURGERY_N_MAX - 1, "steady-state map", "nx + nu <= FB_SURGERY_N_MAX")) return rc;
    if (int32_t rc = verb_model(verb, h)) return rc;
    if (int32_t rc = verb_continuous(verb, h)) return rc;
    return steady_run(verb, h, false, iz, nz, K, nullptr, k_per_system, X, U, nullptr, K_fwd, rpiv, status);
}

}  // extern "C"
