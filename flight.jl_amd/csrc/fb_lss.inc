// fb_lss.inc — Model(lss): LinearizedSS handles (include/flightbatch.h: FB_MODEL_LSS, fb_lss_create, fb_lss_set_model,
// fb_lss_from_linearization; kernels: lss_kernels.hpp; docs/design/linearize.md, "Model(lss) on the device"). Included by fb_capi.hip.
// Reference: FP/linearization.jl:157-192 — a LinearizedSS is a ModelDefinition with X = copy(x0), U = copy(u0), @no_step, @no_periodic
// and f_ode!: xdot = xdot0 + A (x - x0) + B (u - u0), y = y0 + C (x - x0) + D (u - u0).
// The state, input, output and derivative rows are the handle's x, u, y, xdot in the ABI's layout [rows x n], so that the state copies and the
// device log work on them as on any other model; the model itself is the handle's own copy in the layout stated at fbg::ab_index (lss_group.hpp).
// First comes what every verb of the family shares on the host (docs/design/linearize.md, "What the family shares").

struct LssState {
    int nx = 0, nu = 0, ny = 0, G = 0;
    int xch = 0;                 // the stepper's exchange: 0 LDS panel, 1 cross-lane reads (FLIGHTBATCH_LSS_EXCHANGE, A/B switch for measurements)
    double *ab = nullptr, *xs = nullptr, *u0 = nullptr, *y0 = nullptr, *cd = nullptr;
    bool have_model = false;
    double Ts = 0;               // > 0: a sampled model made by fb_lss_c2d (fb_c2d.inc): Phi, Gamma and delta in the places of A, B and xdot0
};
// blocks of lin_buf that the last lin_run wrote (fb_handle_s::lin_have)
enum { LIN_HAVE_BASE = 1, LIN_HAVE_X0 = 2, LIN_HAVE_U0 = 4, LIN_HAVE_AB = 8, LIN_HAVE_CD = 16 };

static bool is_lss(fb_handle h) { return h->model == FB_MODEL_LSS; }
// verbs of other model families on a LinearizedSS handle
static int32_t lss_refuse(const char* verb, const char* why) {
    return fail("%s: not defined for a LinearizedSS handle (FB_MODEL_LSS): %s", verb, why);
}
// the group size of the verbs with 8 / 16 / 32 instances: the smallest with a lane per row (the stepper's own has 4 as well)
static int group_for(int rows) { return rows <= 8 ? 8 : rows <= 16 ? 16 : 32; }
static int lss_group(int nx) { return nx <= 4 ? 4 : group_for(nx); }

// `launch` between a pair of per-launch timing stamps of h, when those are on and the window has room (fb_timing_begin_per_launch)
template <class F>
static int32_t stamped(fb_handle h, F&& launch) {
    const bool stamp = h->timing && h->lev_used < h->lev_max;
    if (stamp) HIPCHK(hipEventRecord(h->lev[2 * h->lev_used], h->stream));
    launch();
    if (stamp) { HIPCHK(hipEventRecord(h->lev[2 * h->lev_used + 1], h->stream)); h->lev_used++; }
    return 0;
}
// a verb's kernel on h's stream, stamped: `groups` groups of P lanes, 64 / P to a one-wave workgroup; kernel(P) = [](auto P) { return k<P.value>; }
template <class Args, class K>
static int32_t family_launch(fb_handle h, int P, int64_t groups, const Args& a, K&& kernel) {
    using std::integral_constant;
    void (*const k)(Args) = P == 8 ? kernel(integral_constant<int, 8>{}) : P == 16 ? kernel(integral_constant<int, 16>{}) : kernel(integral_constant<int, 32>{});
    const dim3 grid = grid_for(groups, fbg::WAVE / P), block(fbg::WAVE);
    if (int32_t rc = stamped(h, [&] { hipLaunchKernelGGL(k, grid, block, 0, h->stream, a); })) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

// the device blocks of one call: freed when the call returns, on every path; g_err stays as the step that failed left it
struct DevBlocks {
    std::vector<void*> held;
    ~DevBlocks() { for (void* p : held) (void)hipFree(p); }
    template <class T> int32_t alloc(T** out, size_t count) { HIPCHK(hipMalloc(out, sizeof(T) * count)); held.push_back(*out); return 0; }
};
// a handle in the making: destroyed when the call returns, with the failing step's reason kept, unless it was handed over
struct NewHandle {
    fb_handle h = nullptr;
    ~NewHandle() { if (h) { const std::string msg = g_err; fb_destroy(h); g_err = msg; } }
    fb_handle release() { fb_handle r = h; h = nullptr; return r; }
};

// what a design verb asks of its handle, in this order; then, where the verb's own order of checks puts it, that it has a model
static int32_t verb_handle(const char* verb, fb_handle h, int nx_max, const char* takes, const char* limit) {
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("%s: the handle is not a LinearizedSS handle (FB_MODEL_LSS: fb_lss_create, fb_lss_from_linearization)", verb);
    const LssState* L = h->lss;
    if (!L) return fail("%s: the handle is not ready (its creation did not finish)", verb);
    if (L->nx < 1 || L->nx > nx_max) return fail("%s: nx = %d, the %s takes 1 <= nx <= %d (%s)", verb, L->nx, takes, nx_max, limit);
    return 0;
}
static int32_t verb_model(const char* verb, fb_handle h) {
    return h->lss->have_model ? 0 : fail("%s: this LinearizedSS handle has no model yet (fb_lss_set_model)", verb);
}
// the design verbs read A and B as a continuous-time model: a sampled handle (fb_lss_c2d) is refused before anything is launched
static int32_t verb_continuous(const char* verb, fb_handle h) {
    return h->lss->Ts > 0.0 ? fail("%s: a continuous-time verb on a sampled model (this handle was made by fb_lss_c2d, Ts = %g)", verb, h->lss->Ts) : 0;
}
// the model's fields of a verb's argument struct from the handle: [A | B] with its sizes; for a verb on a channel also [C | D], nu and ny
template <class A> static void verb_args_ab(A& a, fb_handle h) { a.ab = h->lss->ab; a.n = h->n; a.nx = h->lss->nx; a.G = h->lss->G; }
template <class A> static void verb_args(A& a, fb_handle h) { verb_args_ab(a, h); a.cd = h->lss->cd; a.nu = h->lss->nu; a.ny = h->lss->ny; }
// a list of a verb's arguments against its limit (a NULL list stands for "all of them" and passes); false with the refusal set
static bool lists_in_range(const char* verb, const int32_t* list, int cnt, int lim, const char* what) {
    for (int k = 0; list && k < cnt; k++)
        if (list[k] < 0 || list[k] >= lim) { fail("%s: %s[%d] = %d is outside [0, %d)", verb, what, k, (int)list[k], lim); return false; }
    return true;
}
// a staged model of n systems on the host (the layout: fbg::staged_index, lss_group.hpp): where its blocks begin, in doubles from its
// base (xdot0 at 0), what it takes in all, and what k_lss_gather reads of one that lies at `base`
struct Staged {
    int nx, nu, ny;
    size_t x0, u0, y0, AB, CD, doubles;
    Staged(int nx_, int nu_, int ny_, int64_t n) : nx(nx_), nu(nu_), ny(ny_) {
        const size_t un = (size_t)n;
        x0 = nx * un; u0 = x0 + nx * un; y0 = u0 + nu * un; AB = y0 + ny * un; CD = AB + (size_t)nx * (nx + nu) * un;
        doubles = CD + (size_t)ny * (nx + nu) * un;
    }
    fbl::LssSrc src(const double* base) const { return {base, base + x0, base + u0, base + y0, base + AB, base + CD, nx, nu, ny, nullptr}; }
};
static int lss_exchange() { const char* e = getenv("FLIGHTBATCH_LSS_EXCHANGE"); return e && !strcmp(e, "shfl") ? 1 : 0; }

static fbl::LssArgs lss_args(fb_handle h) {
    const LssState* L = h->lss;
    fbl::LssArgs a;
    a.ab = L->ab; a.xs = L->xs; a.u0 = L->u0; a.y0 = L->y0; a.cd = L->cd;
    a.x = h->x; a.u = h->u; a.y = h->y; a.xdot = nullptr;
    a.n = h->n; a.nx = L->nx; a.nu = L->nu; a.ny = L->ny; a.dt = h->params.dt;
    return a;
}
static dim3 lss_grid(fb_handle h) { return grid_for(h->n, fbl::LSS_BLOCK / h->lss->G); }
template <class F>
static void lss_with_group(const LssState* L, F&& f) {
    switch (L->G) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        default: f(std::integral_constant<int, 32>{}); break;
    }
}
static int32_t lss_create(fb_handle h, int nx, int nu, int ny) {
    LssState* L = new LssState();
    h->lss = L;
    L->nx = nx; L->nu = nu; L->ny = ny; L->G = lss_group(nx); L->xch = lss_exchange();
    const size_t n = (size_t)h->n, S = n * L->G;
    HIPCHK(hipMalloc(&L->ab, sizeof(double) * (L->G + nu) * S));
    HIPCHK(hipMalloc(&L->xs, sizeof(double) * 2 * S));
    HIPCHK(hipMalloc(&L->u0, sizeof(double) * nu * n));
    HIPCHK(hipMalloc(&L->y0, sizeof(double) * ny * n));
    HIPCHK(hipMalloc(&L->cd, sizeof(double) * (nx + nu) * ny * n));
    HIPCHK(hipMalloc(&h->x_own, sizeof(double) * nx * n));
    HIPCHK(hipMalloc(&h->u, sizeof(double) * nu * n));
    HIPCHK(hipMalloc(&h->y, sizeof(double) * ny * n));
    HIPCHK(hipMalloc(&h->xdot, sizeof(double) * nx * n));
    HIPCHK(hipMalloc(&h->status, sizeof(int32_t) * n));
    HIPCHK(hipMalloc(&h->term_step, sizeof(long long) * n));
    HIPCHK(hipMalloc(&h->term_where, sizeof(int32_t) * n));
    h->x = h->x_own;
    HIPCHK(hipMemsetAsync(h->x, 0, sizeof(double) * nx * n, h->stream));
    HIPCHK(hipMemsetAsync(h->u, 0, sizeof(double) * nu * n, h->stream));
    HIPCHK(hipMemsetAsync(h->y, 0, sizeof(double) * ny * n, h->stream));
    HIPCHK(hipMemsetAsync(h->status, 0, sizeof(int32_t) * n, h->stream));   // (a linear model throws nothing: the words stay 0 unless fb_set_status writes them)
    HIPCHK(hipMemsetAsync(h->term_step, 0, sizeof(long long) * n, h->stream));
    HIPCHK(hipMemsetAsync(h->term_where, 0, sizeof(int32_t) * n, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
static void lss_destroy(fb_handle h) {
    LssState* L = h->lss;
    if (!L) return;
    (void)hipFree(L->ab); (void)hipFree(L->xs); (void)hipFree(L->u0); (void)hipFree(L->y0); (void)hipFree(L->cd);
    delete L;
    h->lss = nullptr;
}
static int32_t lss_ready(fb_handle h) {
    if (!h->lss->have_model) return fail("this LinearizedSS handle has no model yet (fb_lss_set_model)");
    return 0;
}
static int32_t lss_rows(fb_handle h, double* dev, const double* host_in, double* host_out, int rows) {
    const size_t bytes = sizeof(double) * (size_t)rows * h->n;
    if (host_in) HIPCHK(hipMemcpyAsync(dev, host_in, bytes, hipMemcpyHostToDevice, h->stream));
    if (host_out) HIPCHK(hipMemcpyAsync(host_out, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
static int32_t lss_f_ode(fb_handle h, double* xdot) {
    if (int32_t rc = lss_ready(h)) return rc;
    if (xdot && h->lss->Ts > 0.0) return fail("fb_f_ode: a sampled model (fb_lss_c2d) has no derivative: pass xdot = NULL to refresh the outputs");
    fbl::LssArgs a = lss_args(h);
    a.xdot = xdot ? h->xdot : nullptr;
    lss_with_group(h->lss, [&](auto G) { hipLaunchKernelGGL(fbl::k_lss_f_ode<G.value>, lss_grid(h), dim3(fbl::LSS_BLOCK), 0, h->stream, a); });
    HIPCHK(hipGetLastError());
    if (xdot) return lss_rows(h, h->xdot, nullptr, xdot, h->lss->nx);
    return 0;
}
// nsteps of k_lss_rk4, or of k_lss_map on a sampled handle (whose step is Ts), steps_per_launch to a launch; u is held over the call, t is
// advanced here
static int32_t lss_step(fb_handle h, int64_t nsteps) {
    const LssState* L = h->lss;
    const bool sampled = L->Ts > 0.0;
    if (sampled && memcmp(&h->params.dt, &L->Ts, sizeof(double)) != 0)
        return fail("fb_step: this handle is a sampled model with Ts = %.17g (fb_lss_c2d) and its dt was changed to %.17g: a sampled model steps by its own sample time only", L->Ts, h->params.dt);
    const fbl::LssArgs a = lss_args(h);
    int64_t left = nsteps;
    while (left > 0) {
        const int k = (int)(left < h->steps_per_launch ? left : h->steps_per_launch);
        const int32_t rc = stamped(h, [&] {
            lss_with_group(L, [&](auto G) {
                if (!sampled) {
                    if (L->xch == 0) hipLaunchKernelGGL((fbl::k_lss_rk4<G.value, 0>), lss_grid(h), dim3(fbl::LSS_BLOCK), 0, h->stream, a, k);
                    else hipLaunchKernelGGL((fbl::k_lss_rk4<G.value, 1>), lss_grid(h), dim3(fbl::LSS_BLOCK), 0, h->stream, a, k);
                }
                else if (L->xch == 0) hipLaunchKernelGGL((fbz::k_lss_map<G.value, 0>), lss_grid(h), dim3(fbl::LSS_BLOCK), 0, h->stream, a, k);
                else hipLaunchKernelGGL((fbz::k_lss_map<G.value, 1>), lss_grid(h), dim3(fbl::LSS_BLOCK), 0, h->stream, a, k);
            });
        });
        if (rc) return rc;
        left -= k;
        h->steps_done += k;
        h->launches++;
    }
    HIPCHK(hipGetLastError());
    h->t += (double)nsteps * h->params.dt;
    return 0;
}
// the handle's copy of the model from a linearisation result on ITS device (`s`, in fb_linearize's layout), through the index lists
// (host, checked by the caller); leaves x = x0, u = u0, t = 0, step count 0
static int32_t lss_gather(fb_handle h, fbl::LssSrc s, const int32_t* ix, const int32_t* iu, const int32_t* iy) {
    LssState* L = h->lss;
    std::vector<int32_t> idx;
    for (int k = 0; k < L->nx; k++) idx.push_back(ix ? ix[k] : k);
    for (int k = 0; k < L->nu; k++) idx.push_back(iu ? iu[k] : k);
    for (int k = 0; k < L->ny; k++) idx.push_back(iy ? iy[k] : k);
    DevBlocks blocks;
    int32_t* d_idx = nullptr;
    if (int32_t rc = blocks.alloc(&d_idx, idx.size())) return rc;
    HIPCHK(hipMemcpyAsync(d_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, h->stream));
    s.idx = d_idx;
    const fbl::LssDst d = {L->ab, L->xs, L->u0, L->y0, L->cd, h->x, h->u, L->nx, L->nu, L->ny, L->G, h->n};
    hipLaunchKernelGGL(fbl::k_lss_gather, grid_for(h->n, fbl::LSS_BLOCK), dim3(fbl::LSS_BLOCK), 0, h->stream, s, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    L->have_model = true;
    h->t = 0.0; h->steps_done = 0;
    if (h->log) h->log->step_index = 0;
    return 0;
}
// [A | B] or [C | D] (`cd`) of the handle's copy into fb_linearize's layout, M | N; at(L, n, i, r, c): the kernels' index of (r, c) of system i
template <class At>
static int32_t lss_unpad(const char* verb, fb_handle h, bool cd, double* M, double* N, At at) {
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("%s: the handle is not a LinearizedSS handle (fb_lss_create)", verb);
    if (int32_t rc = lss_ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const LssState* L = h->lss;
    const int64_t n = h->n;
    const int nx = L->nx, nu = L->nu, rows = cd ? L->ny : nx;
    std::vector<double> buf((size_t)(cd ? (nx + nu) * L->ny : (L->G + nu) * L->G) * n);
    HIPCHK(hipMemcpyAsync(buf.data(), cd ? L->cd : L->ab, sizeof(double) * buf.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < nx + nu; c++) {
        double* out = c < nx ? M : N;
        if (!out) continue;
        for (int r = 0; r < rows; r++)
            for (int64_t i = 0; i < n; i++) out[fbg::staged_index(n, i, rows, r, c < nx ? c : c - nx)] = buf[at(L, n, i, r, c)];
    }
    return 0;
}
// sizes are checked before anything touches a device
static int32_t lss_check_dims(int32_t nx, int32_t nu, int32_t ny, int64_t n) {
    if (nx < 1 || nx > fbl::LSS_NX_MAX) return fail("fb_lss_create: nx = %d, a LinearizedSS handle takes 1 <= nx <= %d", (int)nx, fbl::LSS_NX_MAX);
    if (nu < 1 || nu > fbl::LSS_NU_MAX) return fail("fb_lss_create: nu = %d, a LinearizedSS handle takes 1 <= nu <= %d", (int)nu, fbl::LSS_NU_MAX);
    if (ny < 1 || ny > fbl::LSS_NY_MAX) return fail("fb_lss_create: ny = %d, a LinearizedSS handle takes 1 <= ny <= %d", (int)ny, fbl::LSS_NY_MAX);
    if (n <= 0) return fail("n must be positive");
    if (n > ((int64_t)1 << 31) - 1) return fail("fb_lss_create: n = %lld exceeds the 2^31 - 1 systems of one launch grid", (long long)n);
    return 0;
}
static int32_t lss_new_handle(int32_t nx, int32_t nu, int32_t ny, int64_t n, int32_t device_id, fb_handle* out) {
    HIPCHK(hipSetDevice(device_id));
    NewHandle made;
    fb_handle h = made.h = new fb_handle_s();
    h->model = FB_MODEL_LSS; h->kin = FB_KIN_WA; h->dtype = FB_F64; h->device = device_id; h->n = n;
    h->params.dt = 0.02; h->params.periodic_n = 1; h->params.surface = 0;
    h->params.T_sl = isa::T_std; h->params.p_sl = isa::p_std;
    h->params.wind_ned[0] = h->params.wind_ned[1] = h->params.wind_ned[2] = 0.0;
    h->params.h_terrain = 0.0;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return fail("fb_lss_create: hipStreamCreateWithFlags failed");
    h->stream = h->own_stream;
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) return fail("fb_lss_create: hipEventCreate failed");
    if (int32_t rc = lss_create(h, nx, nu, ny)) return rc;
    *out = made.release();
    return 0;
}
// The tail of every verb that makes a handle from a staged model `s` on src's device (src: the vehicle handle that was linearised, the
// plant, the model that was transformed): `made`, from lss_new_handle, gets its copy of the model through the index lists (host, checked
// by the caller) once src's stream has written `s`, takes src's dt, and is handed over. A source that runs on its caller's stream: so
// does the model made from it.
static int32_t lss_adopt(fb_handle src, NewHandle& made, const fbl::LssSrc& s, const int32_t* ix, const int32_t* iu, const int32_t* iy, fb_handle* out) {
    HIPCHK(hipStreamSynchronize(src->stream));   // (the staged model the new handle's stream is about to read; the verb's copies to the host)
    if (int32_t rc = lss_gather(made.h, s, ix, iu, iy)) return rc;
    made.h->params.dt = src->params.dt;
    if (src->stream != src->own_stream) made.h->stream = src->stream;
    *out = made.release();
    return 0;
}

extern "C" {

int32_t fb_lss_create(int32_t nx, int32_t nu, int32_t ny, int64_t n, int32_t device_id, fb_handle* out) {
    if (!out) return fail("out is null");
    *out = nullptr;
    if (int32_t rc = lss_check_dims(nx, nu, ny, n)) return rc;
    if (device_id < 0) return fail("device_id < 0: libflightbatch has no CPU backend");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available: libflightbatch requires a GPU");
    if (device_id >= ndev) return fail("device_id out of range");
    return lss_new_handle(nx, nu, ny, n, device_id, out);
}

int32_t fb_lss_set_model(fb_handle h, const double* xdot0, const double* x0, const double* u0, const double* y0,
                         const double* A, const double* B, const double* C, const double* D) {
    if (!h) return fail("null handle");
    if (!is_lss(h)) return fail("fb_lss_set_model: the handle is not a LinearizedSS handle (fb_lss_create)");
    if (h->lss && h->lss->Ts > 0.0) return fail("fb_lss_set_model: the handle is a sampled model made by fb_lss_c2d: its model is not replaced (discretise the new model instead)");
    if (!xdot0 || !x0 || !u0 || !y0 || !A || !B || !C || !D) return fail("fb_lss_set_model: every block of the model is required");
    HIPCHK(hipSetDevice(h->device));
    const LssState* L = h->lss;
    const int64_t n = h->n, nx = L->nx, nu = L->nu, ny = L->ny;
    // staged on the device in the layout fb_linearize writes, then k_lss_gather with every index: one path for both ways in
    const Staged staged(L->nx, L->nu, L->ny, n);
    DevBlocks blocks;
    double* st = nullptr;
    if (int32_t rc = blocks.alloc(&st, staged.doubles)) return rc;
    double* p = st;
    int32_t rc = 0;
    auto put = [&](const double* host, int64_t rows) {   // (the blocks in the staged order: B behind A, D behind C)
        if (!rc && hipMemcpyAsync(p, host, sizeof(double) * rows * n, hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail("fb_lss_set_model: copying the model to the device failed");
        p += rows * n;
    };
    put(xdot0, nx); put(x0, nx); put(u0, nu); put(y0, ny);
    put(A, nx * nx); put(B, nx * nu);
    put(C, ny * nx); put(D, ny * nu);
    const fbl::LssSrc s = staged.src(st);
    if (!rc) rc = lss_gather(h, s, nullptr, nullptr, nullptr);
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

int32_t fb_lss_exchange(fb_handle h, int32_t* xch) {
    if (!h) return fail("fb_lss_exchange: null handle");
    if (!is_lss(h)) return fail("fb_lss_exchange: the handle is not a LinearizedSS handle (fb_lss_create, fb_lss_from_linearization)");
    if (!xch) return fail("fb_lss_exchange: xch is null");
    *xch = h->lss->xch;
    return 0;
}

int32_t fb_lss_from_linearization(fb_handle src, const int32_t* ix, int32_t nx, const int32_t* iu, int32_t nu, const int32_t* iy, int32_t ny, fb_handle* out) {
    if (!out) return fail("out is null");
    *out = nullptr;
    if (!src) return fail("null handle");
    if (is_lss(src)) return lss_refuse("fb_lss_from_linearization", "the source is a vehicle handle that fb_linearize or fb_linearize_state has run on");
    if (!src->lin_buf || !(src->lin_have & LIN_HAVE_BASE))
        return fail("fb_lss_from_linearization: no linearisation has run on the source handle (fb_linearize, fb_linearize_state)");
    const int snx = src->lin_nx, snu = src->lin_nu, sny = src->lin_ny;
    static const struct { int bit; const char* what; } need[4] = {{LIN_HAVE_X0, "x0"}, {LIN_HAVE_U0, "u0"}, {LIN_HAVE_AB, "A | B"}, {LIN_HAVE_CD, "C | D"}};
    for (const auto& b : need)
        if (!(src->lin_have & b.bit))
            return fail("fb_lss_from_linearization: the source handle's last linearisation did not write %s on the device (its caller passed NULL for that block)", b.what);
    if (!ix) nx = snx;
    if (!iu) nu = snu;
    if (!iy) ny = sny;
    if (int32_t rc = lss_check_dims(nx, nu, ny, src->n)) return rc;
    auto in_range = [&](const int32_t* list, int cnt, int lim, const char* what) -> bool {
        for (int k = 0; list && k < cnt; k++)
            if (list[k] < 0 || list[k] >= lim) { fail("fb_lss_from_linearization: %s index %d is outside [0, %d)", what, (int)list[k], lim); return false; }
        return true;
    };
    if (!in_range(ix, nx, snx, "state") || !in_range(iu, nu, snu, "input") || !in_range(iy, ny, sny, "output")) return -1;
    HIPCHK(hipSetDevice(src->device));
    NewHandle made;
    if (int32_t rc = lss_new_handle(nx, nu, ny, src->n, src->device, &made.h)) return rc;
    return lss_adopt(src, made, Staged(snx, snu, sny, src->n).src(src->lin_buf), ix, iu, iy, out);   // (lin_buf: lin_run's rows)
}

}  // extern "C"
