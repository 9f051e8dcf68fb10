// fb_lin.inc — linearize (include/flightbatch.h: fb_linearize, fb_linearize_state, fb_linearize_dims; kernels: lin_kernels.hpp).
// Included at the end of fb_capi.hip.

// the reference has get_x_ss / get_u_ss / get_y_ss for Vehicle{NED} and Robot2D only (c172s.jl:397-400, c172x.jl:452-455, robot2d.jl:253-275)
static int32_t lin_supported(fb_handle h) {
    if (!h) return fail("null handle");
    if (is_lss(h)) return lss_refuse("linearize", "the handle IS a linearisation; the reference defines linearize for vehicles");
    if (h->dtype != FB_F64) return fail("linearize: FB_F32 handles are not supported (the Jacobians are fp64 differences)");
    if (h->model == FB_MODEL_ROBOT2D) return 0;
    if (h->kin != FB_KIN_NED) return fail("linearize: Cessna172Sv0 / Cessna172Xv2 have a state-space model with NED kinematics only (the reference defines get_x_ss for Vehicle{NED})");
    return 0;
}
static void lin_dims_of(fb_handle h, int& nx, int& nu, int& ny) {
    if (h->model == FB_MODEL_ROBOT2D) { nx = 4; nu = 1; ny = 6; }
    else if (is_x2(h)) { nx = LinDims<true>::NX; nu = LinDims<true>::NU; ny = LinDims<true>::NY; }
    else { nx = LinDims<false>::NX; nu = LinDims<false>::NU; ny = LinDims<false>::NY; }
}
// the environment of Linearization.linearize(vehicle, trim_params): SimpleAtmosphere(; wind = NoWind()) at the ISA sea level and
// HorizontalTerrain() (elevation 0, DryTarmac) (aircraftbase.jl:300-301, terrain.jl:34-38), whatever the handle's params or rows say
static KArgs still_air_args(fb_handle h) {
    KArgs a = make_args(h);
    const double T = isa::T_std, p = isa::p_std;
    a.env = {T, p, 0.0, 0.0, 0.0, 0.0, 0, log(p / 101325.0), exp(0.5 * 6.5e-3 * 287.05287 / 9.80665 * log(p / 101325.0)) / sqrt(T)};   // (make_args' expressions)
    a.env_rows = nullptr;
    return a;
}
struct LinHost { double *xdot0, *x0, *u0, *y0, *A, *B, *C, *D; int32_t* status; };

// base launch, difference launch, copies of the requested blocks
static int32_t lin_run(fb_handle h, const KArgs& a, int32_t scheme, const LinHost& out) {
    const int64_t n = h->n;
    int nx, nu, ny;
    lin_dims_of(h, nx, nu, ny);
    const int nc = nx + nu;
    const bool two = scheme == FB_LIN_ONESIDED2 && h->model != FB_MODEL_ROBOT2D;   // (the first points' results: as many rows again as A|B and C|D)
    const size_t need = (size_t)(2 * nx + nu + ny + (two ? 2 : 1) * (nx + ny) * nc) * (size_t)n;
    if (!h->lin_buf || h->lin_doubles < need) {
        hipFree(h->lin_buf); h->lin_buf = nullptr; h->lin_doubles = 0;
        HIPCHK(hipMalloc(&h->lin_buf, sizeof(double) * need));
        h->lin_doubles = need;
    }
    if (!h->lin_st) HIPCHK(hipMalloc(&h->lin_st, sizeof(int32_t) * n));
    double* xdot0 = h->lin_buf;
    double* x0 = xdot0 + (int64_t)nx * n;
    double* u0 = x0 + (int64_t)nx * n;
    double* y0 = u0 + (int64_t)nu * n;
    double* AB = y0 + (int64_t)ny * n;
    double* CD = AB + (int64_t)nx * nc * n;
    double* tAB = CD + (int64_t)ny * nc * n;
    double* tCD = tAB + (int64_t)nx * nc * n;
    const bool want_ab = out.A || out.B, want_cd = out.C || out.D;
    h->lin_have = 0;   // (set again below, once the launches are queued; what fb_lss_from_linearization may read)
    const dim3 gb = grid_for(n, 256), gd(gb.x, (unsigned)nc);
    if (h->model == FB_MODEL_ROBOT2D) {
        HIPCHK(hipMemsetAsync(h->lin_st, 0, sizeof(int32_t) * n, h->stream));   // (Robot2D's f_ode! throws nothing)
        const fbr::R2LinOut o = {xdot0, out.x0 ? x0 : nullptr, out.u0 ? u0 : nullptr, y0, want_ab ? AB : nullptr, want_cd ? CD : nullptr, scheme};
        const fbr::R2Args<double> ra = r2_args<double>(h, h->r2);
        hipLaunchKernelGGL(fbr::k_r2_lin_base, gb, dim3(256), 0, h->stream, ra, o);
        if (want_ab || want_cd) {
            if (scheme == FB_LIN_FORWARD) hipLaunchKernelGGL(fbr::k_r2_lin_diff<FB_LIN_FORWARD>, gd, dim3(256), 0, h->stream, ra, o);
            else hipLaunchKernelGGL(fbr::k_r2_lin_diff<FB_LIN_ONESIDED2>, gd, dim3(256), 0, h->stream, ra, o);
        }
    } else {
        const LinOut o = {xdot0, out.x0 ? x0 : nullptr, out.u0 ? u0 : nullptr, y0, want_ab ? AB : nullptr, want_cd ? CD : nullptr,
                          two ? tAB : nullptr, two ? tCD : nullptr, h->lin_st, scheme};
        auto launch = [&](auto X_) {
            constexpr bool X = decltype(X_)::value;
            hipLaunchKernelGGL(k_lin_base<X>, gb, dim3(256), 0, h->stream, a, o);
            if (!want_ab && !want_cd) return;
            if (scheme == FB_LIN_FORWARD) { hipLaunchKernelGGL((k_lin_diff<X, FB_LIN_FORWARD, 0>), gd, dim3(256), 0, h->stream, a, o); return; }
            hipLaunchKernelGGL((k_lin_diff<X, FB_LIN_ONESIDED2, 0>), gd, dim3(256), 0, h->stream, a, o);
            hipLaunchKernelGGL((k_lin_diff<X, FB_LIN_ONESIDED2, 1>), gd, dim3(256), 0, h->stream, a, o);
        };
        if (is_x2(h)) launch(std::true_type{});
        else launch(std::false_type{});
    }
    HIPCHK(hipGetLastError());
    h->lin_have = LIN_HAVE_BASE | (out.x0 ? LIN_HAVE_X0 : 0) | (out.u0 ? LIN_HAVE_U0 : 0) | (want_ab ? LIN_HAVE_AB : 0) | (want_cd ? LIN_HAVE_CD : 0);
    h->lin_nx = nx; h->lin_nu = nu; h->lin_ny = ny;
    auto get = [&](double* host, const double* dev, int64_t rows) -> int32_t {
        if (host) HIPCHK(hipMemcpyAsync(host, dev, sizeof(double) * rows * n, hipMemcpyDeviceToHost, h->stream));
        return 0;
    };
    if (int32_t rc = get(out.xdot0, xdot0, nx)) return rc;
    if (int32_t rc = get(out.x0, x0, nx)) return rc;
    if (int32_t rc = get(out.u0, u0, nu)) return rc;
    if (int32_t rc = get(out.y0, y0, ny)) return rc;
    if (int32_t rc = get(out.A, AB, (int64_t)nx * nx)) return rc;
    if (int32_t rc = get(out.B, AB + (int64_t)nx * nx * n, (int64_t)nx * nu)) return rc;
    if (int32_t rc = get(out.C, CD, (int64_t)ny * nx)) return rc;
    if (int32_t rc = get(out.D, CD + (int64_t)ny * nx * n, (int64_t)ny * nu)) return rc;
    if (out.status) HIPCHK(hipMemcpyAsync(out.status, h->lin_st, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" {

int32_t fb_linearize_dims(fb_handle h, int32_t* nx, int32_t* nu, int32_t* ny) {
    if (int32_t rc = lin_supported(h)) return rc;
    int a, b, c;
    lin_dims_of(h, a, b, c);
    if (nx) *nx = a;
    if (nu) *nu = b;
    if (ny) *ny = c;
    return 0;
}

int32_t fb_linearize(fb_handle h, const double* params, double* trim_state, int32_t* success, double* cost, int32_t scheme,
                     double* xdot0, double* x0, double* u0, double* y0, double* A, double* B, double* C, double* D, int32_t* lin_status) {
    if (int32_t rc = lin_supported(h)) return rc;
    if (scheme != FB_LIN_FORWARD && scheme != FB_LIN_ONESIDED2) return fail("linearize: unknown difference scheme %d", (int)scheme);
    const LinHost out = {xdot0, x0, u0, y0, A, B, C, D, lin_status};
    if (h->model == FB_MODEL_ROBOT2D) {   // linearize(mdl, ip): f_init!(mdl, ip), the Jacobians, f_init! again (robot2d.jl:315-341)
        if (int32_t rc = r2_ready(h)) return rc;
        HIPCHK(hipSetDevice(h->device));
        std::vector<double> zeros;
        if (!params) { zeros.assign((size_t)FB_R2_NINIT * h->n, 0.0); params = zeros.data(); }   // InitParameters()
        if (int32_t rc = r2_f_init(h, params, FB_R2_NINIT)) return rc;
        return lin_run(h, make_args(h), scheme, out);
    }
    if (int32_t rc = check_ready_x2(h)) return rc;
    if (!params || !trim_state) return fail("linearize: trim parameters and the trim-state guess are required for this model");
    HIPCHK(hipSetDevice(h->device));
    fsal_invalidate(h);
    const KArgs a = still_air_args(h);
    if (int32_t rc = trim_run(h, a, params, trim_state, success, cost)) return rc;
    return lin_run(h, a, scheme, out);
}

int32_t fb_linearize_state(fb_handle h, int32_t scheme, double* xdot0, double* x0, double* u0, double* y0,
                           double* A, double* B, double* C, double* D, int32_t* lin_status) {
    if (int32_t rc = lin_supported(h)) return rc;
    if (scheme != FB_LIN_FORWARD && scheme != FB_LIN_ONESIDED2) return fail("linearize: unknown difference scheme %d", (int)scheme);
    if (h->model == FB_MODEL_ROBOT2D) {
        if (int32_t rc = r2_ready(h)) return rc;
    } else if (int32_t rc = check_ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    return lin_run(h, make_args(h), scheme, {xdot0, x0, u0, y0, A, B, C, D, lin_status});
}

}  // extern "C"
