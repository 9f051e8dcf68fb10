// lin_kernels.hpp — linearize(f, h, x0, u0) on the device (FP/linearization.jl:55-111, FP/aircraftbase.jl:292-334,
// FA/robot2d/robot2d.jl:315-341): the state-space vectors of Cessna172Sv0(NED) / Cessna172Xv2(NED) (FA/c172/c172s/c172s.jl:269-412,
// FA/c172/c172x/c172x.jl:332-490) and Robot2D, and the forward-difference Jacobians A, B, C, D of ẋ_ss = f(x_ss, u_ss), y_ss = h(x_ss, u_ss).
//
//   k_lin_base<X>          one lane per aircraft: f and h at (x0, u0) -> ẋ0, y0 (the quotients' baseline), x0, u0, the status bits
//   k_lin_diff<X, SCHEME>  grid (aircraft block, column j of [x_ss | u_ss]): every workgroup perturbs ONE component, so the perturbation is
//                          wave-uniform and every store is one coalesced row; a lane evaluates one (FB_LIN_FORWARD) or two (FB_LIN_ONESIDED2)
//                          points and writes column j of A|B and of C|D for its aircraft
//   k_r2_lin_base / k_r2_lin_diff<SCHEME>   the same over robot2d_kernels.hpp's fp64 f_ode
//
// Every evaluation is the ground-capable rhs<NED, true> with a sink whose `full` flag is set, like k_f_ode's PanelSink: the high-clearance
// shortcut and the reduced propeller table that a partial sink enables change the bits of ẋ, and a one-ulp change of f is ~1e-8 of a
// Jacobian entry under the forward scheme. The sink keeps only the y_ss rows and hands each to the kernel's functor at once (no record is
// held in registers across the evaluation).
// Matrices are column-major per aircraft, aircraft index fastest: element (i, r, c) of A at A[(r + nx c) n + i] (include/flightbatch.h).
#pragma once
#include "c172_kernels.hpp"
#include "robot2d_kernels.hpp"

namespace fbd {

template <bool X> struct LinDims {
    static constexpr int NX = X ? 20 : 16, NU = 4, NY = X ? 38 : 33, NC = NX + NU;
    static constexpr int O = X ? 5 : 0;   // offset of the y_ss rows behind the state block (Xv2 inserts n_eng and the four positions)
};
// device row (NED mechanisation) of x_ss component j: p q r ψ θ φ v_x v_y v_z ϕ λ h α_filt β_filt ω_eng fuel [thr_p ail_p ele_p rud_p]
FBD constexpr int lin_x_row(int j) {
    return j < 3 ? FB_X_OMEGA_EB_B + j : j < 6 ? FB_X_Q_WB + (j - 3) : j < 9 ? FB_X_V_EB_B + (j - 6) : j < 12 ? FB_X_Q_WB + 3 + (j - 9)
         : j == 12 ? FB_X_ALPHA_FILT : j == 13 ? FB_X_BETA_FILT : j == 14 ? FB_X_ENG_OMEGA : j == 15 ? FB_X_FUEL : X2_ACT + (j - 16);
}
// u_ss component k of Cessna172Sv0 -> row of u (throttle aileron elevator rudder)
FBD constexpr int lin_u_row(int k) { return k == 0 ? FB_U_THROTTLE : k == 1 ? FB_U_AILERON : k == 2 ? FB_U_ELEVATOR : FB_U_RUDDER; }
FBD double lin_u_sat(int k, double v) { return clampd(v, k == 0 ? 0.0 : -1.0, 1.0); }   // the Ranged types of the inputs u_ss assigns

// FB_LIN_FORWARD: FiniteDiff's default forward step max(√eps |x|, √eps), √eps = 2^-26, not re-rounded.
// FB_LIN_ONESIDED2: h = (x + 1e-6 max(|x|, 1)) - x, exactly representable (tests/reference_lqr.py).
FBD double lin_step(int scheme, double x) {
    constexpr double SQRT_EPS = 1.4901161193847656e-08;
    return scheme == FB_LIN_FORWARD ? fmax(SQRT_EPS * fabs(x), SQRT_EPS) : (x + 1e-6 * fmax(fabs(x), 1.0)) - x;
}

// y_ss rows that are rows of the output record (FB_Y_*) go straight to their row of Y (PanelSink's pattern: nothing is held in registers
// across the evaluation); the rest come from the state and the inputs (lin_y_tail)
template <bool X>
struct LinSink {
    static constexpr bool enabled = true, full = true;
    double* Y;   // &dst[0 * n + i]
    int64_t n;
    bool on;     // wave-uniform (a kernel argument is null or not): h is wanted
    FBD void to(int r, double v) const { if (on) Y[(int64_t)r * n] = v; }
    FBD void put(int k, double v) const {
        constexpr int O = LinDims<X>::O;
        switch (k) {
            case FB_Y_KIN + 28: to(0, v); break;  case FB_Y_KIN + 29: to(1, v); break;  case FB_Y_KIN + 30: to(2, v); break;   // ω_eb_b
            case FB_Y_KIN + 0: to(3, v); break;   case FB_Y_KIN + 1: to(4, v); break;   case FB_Y_KIN + 2: to(5, v); break;    // e_nb
            case FB_Y_KIN + 31: to(6, v); break;  case FB_Y_KIN + 32: to(7, v); break;  case FB_Y_KIN + 33: to(8, v); break;   // v_eb_b
            case FB_Y_KIN + 15: to(9, v); break;  case FB_Y_KIN + 16: to(10, v); break; case FB_Y_KIN + 20: to(11, v); break;  // ϕ λ h_e
            case FB_Y_DYN + 31: to(16 + O, v); break; case FB_Y_DYN + 32: to(17 + O, v); break; case FB_Y_DYN + 33: to(18 + O, v); break;  // f_c_c
            case FB_Y_AERO + 0: to(19 + O, v); break; case FB_Y_AERO + 1: to(20 + O, v); break;                                 // α β
            case FB_Y_AIR + 20: to(21 + O, v); break; case FB_Y_AIR + 19: to(22 + O, v); break;                                 // EAS TAS
            case FB_Y_KIN + 34: to(23 + O, v); break; case FB_Y_KIN + 35: to(24 + O, v); break;                                 // v_N v_E
            case FB_Y_KIN + 36: to(25 + O, v); to(28 + O, -v); break;                                                           // v_D, c = -v_D
            case FB_Y_KIN + 38: to(26 + O, v); break; case FB_Y_KIN + 39: to(27 + O, v); break;                                 // χ γ
            default: break;
        }
        // Cessna172Sv0: every other row of the record is computed and used, as fb_f_ode's PanelSink uses it — a value with a second use is
        // not contracted into its consumer (a product that fb_f_ode stores stays a product there) — so that the evaluation rounds as
        // k_f_ode's does. (Cessna172Xv2: the same use trips the spill-placement check in the ISA layer loop of the difference kernel; its
        // evaluations may differ from fb_f_ode's in the last places: docs/design/linearize.md.)
        if constexpr (!X) asm volatile("" ::"v"(v));
    }
};
// the y_ss rows that are states or inputs: α_filt β_filt ω_eng [n_eng] fuel (fuel.x_avail = the state, c172.jl:594-614), [the actuator
// positions pos = Ranged(p), c172x.jl:39-52], the inputs as assigned (Ranged)
template <bool X>
FBD void lin_y_tail(const double (&x)[Dims<X>::NXT], const double (&uss)[4], const LinSink<X>& f) {
    constexpr int O = LinDims<X>::O;
    f.to(12, x[FB_X_ALPHA_FILT]); f.to(13, x[FB_X_BETA_FILT]); f.to(14, x[FB_X_ENG_OMEGA]);
    if constexpr (X) {
        f.to(15, x[FB_X_ENG_OMEGA] / c172::w_rated); f.to(16, x[FB_X_FUEL]);
#pragma unroll
        for (int k = 0; k < 4; k++) f.to(17 + k, lin_u_sat(k, x[X2_ACT + k]));
    } else {
        f.to(15, x[FB_X_FUEL]);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) f.to(29 + O + k, uss[k]);
}

// Cessna172Sv0's inputs with u_ss substituted (steering follows the rudder input as in Inputs::get_steering)
struct InputsLin : Inputs {
    real steer;
    FBD real get_steering() const { return steer; }
};

// One evaluation of f and h at the lane's (x, u_ss): x [NXT] in device rows (already perturbed), uss the four u_ss values as assigned.
// ẋ_ss goes to the rows of dX (&dst[0 * n + i]) when wX, y_ss to those of dY when wY (wX, wY wave-uniform). Returns the status bits.
template <bool X>
FBD int32_t lin_eval(const KArgs& a, int64_t i, const Tables& T, const double (&x)[Dims<X>::NXT], const double (&uss)[4], double* dX, bool wX,
                     double* dY, bool wY) {
    constexpr int NXT = Dims<X>::NXT;
    double xd[NXT];
    StepAux aux;
    auto emit = [&](int j, double v) { xd[j] = v; };
    const LinSink<X> sink{dY, a.n, wY};
    const Env env = env_any(a, i);
    int32_t st;
    if constexpr (X) {
        const InputsX in = {&x[X2_ACT], a.u + i, a.n, a.ui[i]};
        st = rhs<FB_KIN_NED, true>(x, a.s[i], a.s[a.n + i], in, env, T, emit, aux, sink);
#pragma unroll
        for (int k = 0; k < FB_NACT; k++) xd[X2_ACT + k] = 1 / ACT_TAU * ((k < 4 ? uss[k < 4 ? k : 0] : x2_command(a, i, k)) - x[X2_ACT + k]);
    } else {
        double uu[FB_NU];
#pragma unroll
        for (int k = 0; k < FB_NU; k++) uu[k] = a.u[(int64_t)k * a.n + i];
#pragma unroll
        for (int k = 0; k < 4; k++) uu[lin_u_row(k)] = uss[k];
        InputsLin in;
        make_inputs(in, uu, 1, a.ui[i]);
        in.u_glob = a.u + i;
        in.n = a.n;
        in.steer = clampd(clampd(uu[FB_U_RUDDER], -1, 1) + clampd(uu[FB_U_RUDDER_OFFSET], -1, 1), -1, 1);
        st = rhs<FB_KIN_NED, true>(x, a.s[i], a.s[a.n + i], in, env, T, emit, aux, sink);
    }
    if (wX) {
#pragma unroll
        for (int j = 0; j < LinDims<X>::NX; j++) dX[(int64_t)j * a.n] = xd[lin_x_row(j)];
    }
    lin_y_tail<X>(x, uss, sink);
    return st;
}
// x_ss / u_ss of the lane's aircraft at the linearisation point (u_ss: Cessna172Sv0 the Ranged inputs, Cessna172Xv2 the actuator commands)
template <bool X>
FBD void lin_load(const KArgs& a, int64_t i, double (&x)[Dims<X>::NXT], double (&uss)[4]) {
#pragma unroll
    for (int k = 0; k < Dims<X>::NXT; k++) x[k] = a.x[(int64_t)k * a.n + i];
#pragma unroll
    for (int k = 0; k < 4; k++) uss[k] = X ? x2_command(a, i, k) : lin_u_sat(k, a.u[(int64_t)lin_u_row(k) * a.n + i]);
}

struct LinOut {
    double *xdot0, *x0, *u0, *y0;   // [NX|NU|NY x n]; xdot0 and y0 are always given (the quotients' baseline), x0 / u0 may be null
    double *AB, *CD;                // A then B: [NX x NC x n] as A [NX x NX x n] followed by B [NX x NU x n]; C then D likewise; may be null
    double *tAB, *tCD;              // FB_LIN_ONESIDED2: f(z + h) of every column, laid out like AB / CD (the first point's results)
    int32_t* status;                // [n] OR of every evaluation's bits
    int scheme;
};

template <bool X>
__global__ __launch_bounds__(256) void k_lin_base(KArgs a, LinOut o) {
    constexpr int NXT = Dims<X>::NXT;
    __shared__ double lds[LDS_TABLE_DOUBLES];
    __shared__ double rk[LDS_RK_DOUBLES];
    stage_tables<PR_NC>(lds, rk, a.tables);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const Tables T = {(lds_cptr)lds, a.egm96, (lds_cptr)rk, (gk_cptr)a.tables};
    double x[NXT], uss[4];
    lin_load<X>(a, i, x, uss);
    if (o.x0) {
#pragma unroll
        for (int j = 0; j < LinDims<X>::NX; j++) o.x0[(int64_t)j * n + i] = x[lin_x_row(j)];
    }
    if (o.u0) {
#pragma unroll
        for (int k = 0; k < 4; k++) o.u0[(int64_t)k * n + i] = uss[k];
    }
    o.status[i] = lin_eval<X>(a, i, T, x, uss, o.xdot0 + i, true, o.y0 + i, true);
}

// column j = blockIdx.y of [x_ss | u_ss], point PASS of the scheme: z + h (PASS 0) or z + 2h (PASS 1, FB_LIN_ONESIDED2). The evaluation
// writes its raw f and h into the column (FORWARD; ONESIDED2's second point) or into tAB / tCD (ONESIDED2's first point); the quotients
// are formed after it, from what the lane has just written and the base rows: FORWARD (f(z + ε e_j) - f(z)) / ε, ONESIDED2
// (-3 f(z) + 4 f(z + h) - f(z + 2h)) / 2h. (Forming them inside the evaluation, as each row comes out, keeps the loads of the base rows in
// flight across it: 0.1-1.3 KB of scratch.)
template <bool X, int SCHEME, int PASS>
__global__ __launch_bounds__(256) void k_lin_diff(KArgs a, LinOut o) {
    using D = LinDims<X>;
    constexpr int NXT = Dims<X>::NXT;
    __shared__ double lds[LDS_TABLE_DOUBLES];
    __shared__ double rk[LDS_RK_DOUBLES];
    stage_tables<PR_NC>(lds, rk, a.tables);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int j = blockIdx.y;                            // wave-uniform
    const int row = j < D::NX ? lin_x_row(j) : -1;      // device row of the perturbed state, or -1: input j - NX
    const int ku = j - D::NX;
    const Tables T = {(lds_cptr)lds, a.egm96, (lds_cptr)rk, (gk_cptr)a.tables};
    double x[NXT], uss[4];
    lin_load<X>(a, i, x, uss);
    // the perturbed component, read and substituted through unrolled compare chains (no dynamically indexed private array)
    double z0 = 0;
#pragma unroll
    for (int k = 0; k < NXT; k++) if (k == row) z0 = x[k];
#pragma unroll
    for (int k = 0; k < 4; k++) if (k == ku) z0 = uss[k];
    const double h = lin_step(SCHEME, z0);
    const double zp = PASS == 0 ? z0 + h : z0 + 2.0 * h;
#pragma unroll
    for (int k = 0; k < NXT; k++) if (k == row) x[k] = zp;
#pragma unroll
    for (int k = 0; k < 4; k++) if (k == ku) uss[k] = X ? x2_command_sat(k, zp) : lin_u_sat(k, zp);
    const bool to_tmp = SCHEME == FB_LIN_ONESIDED2 && PASS == 0;
    const bool wA = o.AB != nullptr, wC = o.CD != nullptr;   // (kernel arguments: wave-uniform)
    double* const colA = (to_tmp ? o.tAB : o.AB) + (int64_t)D::NX * j * n + i;   // column j of A|B starts at row NX j
    double* const colC = (to_tmp ? o.tCD : o.CD) + (int64_t)D::NY * j * n + i;   // of C|D at row NY j
    const int32_t st = lin_eval<X>(a, i, T, x, uss, colA, wA, colC, wC);
    if (!to_tmp) {
    auto quot = [&](double* col, const double* base, const double* t1, int nr) {
#pragma unroll 1
        for (int r = 0; r < nr; r++) {
            const double f0 = base[(int64_t)r * n + i], v = col[(int64_t)r * n];
            if constexpr (SCHEME == FB_LIN_FORWARD) col[(int64_t)r * n] = (v - f0) / h;
            else col[(int64_t)r * n] = (-3.0 * f0 + 4.0 * t1[(int64_t)r * n] - v) / (2.0 * h);
        }
    };
    constexpr bool TWO = SCHEME == FB_LIN_ONESIDED2;
    if (wA) quot(colA, o.xdot0, TWO ? o.tAB + (int64_t)D::NX * j * n + i : nullptr, D::NX);
    if (wC) quot(colC, o.y0, TWO ? o.tCD + (int64_t)D::NY * j * n + i : nullptr, D::NY);
    }
    if (st) atomicOr(&o.status[i], st);
}

}  // namespace fbd

namespace fbr {
// Robot2D: x_ss = (ω, v, θ, η) = r[0..3], u_ss = u_m = r[4], y_ss = (ω, v, θ, η, u_m, τ_m) (robot2d.jl:233-341)
struct R2LinOut {
    double *xdot0, *x0, *u0, *y0, *AB, *CD;
    int scheme;
};
FBD void r2_lin_eval(const R2Params<double>& p, const double (&z)[5], double (&f)[10]) {
    const double x[4] = {z[0], z[1], z[2], z[3]};
    double xd[4], tm;
    r2_f_ode(p, x, z[4], xd, tm);
    f[0] = xd[0]; f[1] = xd[1]; f[2] = xd[2]; f[3] = xd[3];
    f[4] = z[0]; f[5] = z[1]; f[6] = z[2]; f[7] = z[3]; f[8] = z[4]; f[9] = tm;
}
__global__ __launch_bounds__(256) void k_r2_lin_base(R2Args<double> a, R2LinOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    double z[5], f[10];
#pragma unroll
    for (int k = 0; k < 5; k++) z[k] = a.r[(int64_t)k * n + i];
    r2_lin_eval(a.p, z, f);
#pragma unroll
    for (int k = 0; k < 4; k++) { o.xdot0[(int64_t)k * n + i] = f[k]; if (o.x0) o.x0[(int64_t)k * n + i] = z[k]; }
    if (o.u0) o.u0[i] = z[4];
#pragma unroll
    for (int k = 0; k < 6; k++) o.y0[(int64_t)k * n + i] = f[4 + k];
}
template <int SCHEME>
__global__ __launch_bounds__(256) void k_r2_lin_diff(R2Args<double> a, R2LinOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t n = a.n;
    const int j = blockIdx.y;
    double z[5];
#pragma unroll
    for (int k = 0; k < 5; k++) z[k] = a.r[(int64_t)k * n + i];
    double z0 = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) if (k == j) z0 = z[k];
    const double h = fbd::lin_step(SCHEME, z0);
    double f1[10], f2[10];
    double zp[5];
#pragma unroll
    for (int k = 0; k < 5; k++) zp[k] = k == j ? z0 + h : z[k];
    r2_lin_eval(a.p, zp, f1);
    if constexpr (SCHEME == FB_LIN_ONESIDED2) {
#pragma unroll
        for (int k = 0; k < 5; k++) zp[k] = k == j ? z0 + 2.0 * h : z[k];
        r2_lin_eval(a.p, zp, f2);
    }
    auto q = [&](double v1, double v2, double f0) {
        if constexpr (SCHEME == FB_LIN_FORWARD) return (v1 - f0) / h;
        else return (-3.0 * f0 + 4.0 * v1 - v2) / (2.0 * h);
    };
    if (o.AB) {
#pragma unroll
        for (int r = 0; r < 4; r++) o.AB[(int64_t)(r + 4 * j) * n + i] = q(f1[r], f2[r], o.xdot0[(int64_t)r * n + i]);
    }
    if (o.CD) {
#pragma unroll
        for (int r = 0; r < 6; r++) o.CD[(int64_t)(r + 6 * j) * n + i] = q(f1[4 + r], f2[4 + r], o.y0[(int64_t)r * n + i]);
    }
}
}  // namespace fbr
