/*
 * flightbatch.h — C ABI of libflightbatch: MI355X-native batched 6-DOF flight-dynamics integrator.
 *
 * Drop-in boundary for ONE hot path of e271828e/Flight.jl: the per-step ODE evaluation and fixed-step
 * RK4 integration of `Model(SimpleWorld(Cessna172Sv0()))`, executed for N independent aircraft at once.
 * Every entry point cites the reference interface it stands behind (paths relative to the reference
 * repository root; FC = lib/FlightCore/src, FP = lib/FlightPhysics/src, FA = lib/FlightApps/src).
 * The reference has no FFI for this path (it is pure Julia); the binding a maintainer would add is a
 * `ccall` shim — see INTEGRATION.md, following the in-tree precedent FC/joysticks.jl:45-53.
 *
 * Conventions
 *  - every function returns int32 status: 0 = ok, negative = error (message via fb_last_error()).
 *  - handles are opaque, owned by the library; one handle = one HIP device + one stream.
 *  - host arrays are caller-owned, contiguous, column-major [N x Nfield] with the aircraft index
 *    fastest (structure-of-arrays): element (i, k) lives at ptr[k*N + i].
 *  - calls on one handle are not thread-safe (mirrors the reference's io_lock, FC/sim.jl:545);
 *    different handles may be driven from different threads.
 *  - there is NO CPU fallback: fb_create fails when no HIP device is available.
 */
#ifndef FLIGHTBATCH_H
#define FLIGHTBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fb_handle_s* fb_handle;

/* ---- model / kinematics / dtype ids -------------------------------------------------------- */
enum { FB_MODEL_C172S0 = 0, FB_MODEL_C172X2 = 1, FB_MODEL_ROBOT2D = 2, /* FA/c172/c172s/c172s0.jl:14-18 */
       FB_MODEL_LSS = 3 };  /* Model(lss::LinearizedSS), FP/linearization.jl:157-192: created by fb_lss_create / fb_lss_from_linearization, not by fb_create */
enum { FB_KIN_WA = 0, FB_KIN_ECEF = 1, FB_KIN_NED = 2 };                 /* FP/kinematics.jl:148,250,329   */
/* The kinematic block of x follows the mechanisation (Modeling.X of each, kinematics.jl:152-153, 252-253, 331-332):
 * WA q_wb[4] q_ew[4] h_e (Nx = 27), ECEF q_eb[4] n_e[3] h_e (Nx = 26), NED psi theta phi lat lon h_e (Nx = 24); the blocks
 * before (rows 0-11) and after it (w_eb_b, v_eb_b) are the same. fb_dims reports Nx. */
enum { FB_F64 = 0, FB_F32 = 1 };

/* ---- continuous state x[FB_NX] of Cessna172Sv0 + WA kinematics (SURVEY.md §8 state layout) ---- */
enum {
    FB_X_ALPHA_FILT = 0, FB_X_BETA_FILT = 1, /* FA/c172/c172.jl:296 */
    FB_X_LDG_FRC = 2,                        /* left[2], right[2], nose[2]; FP/landinggear.jl:380-382 */
    FB_X_FUEL = 8,                           /* FA/c172/c172.jl:601 */
    FB_X_ENG_OMEGA = 9, FB_X_ENG_IDLE = 10, FB_X_ENG_FRC = 11, /* FP/piston.jl:290-291 */
    FB_X_Q_WB = 12, FB_X_Q_EW = 16, FB_X_H_E = 20,             /* FP/kinematics.jl:152-153 */
    FB_X_OMEGA_EB_B = 21, FB_X_V_EB_B = 24,                    /* FP/dynamics.jl:436 */
    FB_NX = 27
};
/* ---- discrete state s[FB_NS] (int32) ---- */
enum {
    FB_S_STALL = 0,     /* FA/c172/c172.jl:272-274 */
    FB_S_ENG_STATE = 1, /* FP/piston.jl:198-202 : 0 off, 1 starting, 2 running */
    FB_NS = 2
};
/* ---- real inputs u[FB_NU] ---- */
enum {
    FB_U_THROTTLE = 0, FB_U_MIXTURE = 1,                                  /* FP/piston.jl:259-267 */
    FB_U_AILERON = 2, FB_U_ELEVATOR = 3, FB_U_RUDDER = 4,                 /* FA/c172/c172s/c172s.jl:62-72 */
    FB_U_AILERON_OFFSET = 5, FB_U_ELEVATOR_OFFSET = 6, FB_U_RUDDER_OFFSET = 7,
    FB_U_FLAPS = 8, FB_U_BRAKE_LEFT = 9, FB_U_BRAKE_RIGHT = 10,
    FB_U_M_PILOT = 11, FB_U_M_COPILOT = 12, FB_U_M_LPASS = 13, FB_U_M_RPASS = 14, FB_U_M_BAGGAGE = 15, /* c172.jl:521-527 */
    FB_NU = 16
};
/* ---- integer inputs ui[1]: bit field ---- */
enum {
    FB_UI_ENG_START = 1, FB_UI_ENG_STOP = 2, /* FP/piston.jl:260-261 */
    FB_UI_MIXTURE_AUTO = 4,                  /* FP/piston.jl:263 */
    FB_UI_STEERING_ENGAGED = 8,              /* FP/landinggear.jl:52-55 */
    FB_UI_DEFAULT = 4 | 8,
    FB_NUI = 1
};
/* ---- per-aircraft status word (exceptions of the reference become sticky bits) ---- */
enum {
    FB_ST_OK = 0,
    FB_ST_ALT_RANGE = 1,      /* ArgumentError, FP/geodesy.jl:218-221 */
    FB_ST_ISA_RANGE = 2,      /* ArgumentError, FP/atmosphere.jl:133  */
    FB_ST_GROUND_CRASH = 4,   /* GroundCrash,   FP/landinggear.jl:331-347 */
    FB_ST_NAN = 8,
    FB_ST_CONTACT_ASSERT = 16, /* @assert, FP/landinggear.jl:321 */
    FB_ST_LOST_BALANCE = 32    /* LostBalance, FA/robot2d/robot2d.jl:531-561 (Robot2D only) */
};
/* ---- where a terminated aircraft stopped (fb_get_termination) ----
 * The reference stops a simulation at the first exception (FC/sim.jl:561-570); what it leaves behind is mdl.x / mdl.s as they stand
 * at the throw (sim.x forwards to mdl.x, FC/sim.jl:261-275). A terminated aircraft of the batch is frozen in exactly that condition:
 *   - f_ode! threw (ArgumentError of FP/geodesy.jl:218-221 or FP/atmosphere.jl:133, @assert of FP/landinggear.jl:321) while the
 *     integrator evaluated RK stage k2, k3 or k4 of the step from t_step to t_step + dt: x = the ARGUMENT of that evaluation
 *     (x_step + c dt k_{j-1}; f_ode_wrapper! has copied it into mdl.x, FC/sim.jl:306), s unchanged, `step` RK updates completed;
 *   - f_ode! threw at the new state x_step right after the RK update (OrdinaryDiffEq's evaluation of f at the new u, whose outputs
 *     the callbacks read), before any callback of that step ran: x = x_step;
 *   - f_step! threw (GroundCrash, FP/landinggear.jl:331-347; LostBalance, FA/robot2d/robot2d.jl:553-561) at x_step: x and s carry the
 *     part of f_step! that precedes the throw in the reference's order — quaternion renormalisation (FP/aircraftbase.jl:178), stall
 *     flag (FA/c172/c172.jl:720), the contact-regulator resets of the landing-gear units ahead of the one that threw
 *     (FA/c172/c172.jl:485, FP/landinggear.jl:539-548) — and not what follows it (engine state machine, f_periodic!);
 *   - f_ode! threw at x_step after the step's callbacks had run: the re-evaluation of a state f_step! modified, or the first
 *     evaluation after init / after the host changed the state.
 * The status word holds the single bit of that first exception. (FB_ST_NAN is this library's own check at the end of a launch and
 * has no termination record.) */
enum {
    FB_TERM_NONE = 0,
    FB_TERM_OUTSIDE_STEP = 1,   /* the status bit was not raised by fb_step: a single-call verb (fb_f_ode / fb_f_step) raised it, or the host
                                   set it (fb_set_status) without a record of its own; step = RK updates completed at that moment */
    FB_TERM_F_ODE_K2 = 2,
    FB_TERM_F_ODE_K3 = 3,
    FB_TERM_F_ODE_K4 = 4,
    FB_TERM_F_ODE_NEW = 5,
    FB_TERM_F_STEP = 6,
    FB_TERM_F_ODE_REEVAL = 7
};
/* ---- output record y[FB_NY] (what cb_save logs of `mdl.y`, FC/sim.jl:345-347) ---- */
enum {
    FB_Y_KIN = 0,    /* KinData, 40 doubles, FP/kinematics.jl:46-63:
                        e_nb(psi,theta,phi) q_nb[4] q_eb[4] q_en[4] lat lon n_e[3] h_e h_o r_eb_e[3]
                        w_wb_b[3] w_eb_b[3] v_eb_b[3] v_eb_n[3] v_gnd chi_gnd gamma_gnd */
    FB_Y_AIR = 40,   /* AirData, 22 doubles, FP/atmosphere.jl:198-215:
                        v_ew_n[3] v_ew_b[3] v_wb_b[3] T p rho a mu M Tt pt dp q TAS EAS CAS */
    FB_Y_AERO = 62,  /* 16: alpha beta alpha_filt_dot beta_filt_dot C_D C_Y C_L C_l C_m C_n F[3] tau[3]; c172.jl:276-294 */
    FB_Y_LDG = 78,   /* 3 x 11 (left,right,nose): dh wow xi xi_dot F_dmp_zs wr_b.F[3] wr_b.tau[3]; landinggear.jl:210-222,384-395 */
    FB_Y_PWP = 111,  /* 22: engine MAP f mdot omega tau_shaft P_shaft SFC idle_out frc_out (piston.jl:269-287);
                            propeller J Mt wr_b.F[3] wr_b.tau[3] hr_b[3] P eta_p (propellers.jl:378-390) */
    FB_Y_FUEL = 133, /* 1: m_total; c172.jl:594-598 */
    FB_Y_DYN = 134,  /* 40: mp_b.m mp_b.r_OG[3] mp_b.J[9 row-major] wr_b.F[3] wr_b.tau[3] wdot_eb_b[3] vdot_eb_b[3]
                            a_eb_b[3] a_ib_b[3] f_c_c[3] alpha_ib_b[3] g_c_c[3]; dynamics.jl:416-434 */
    FB_NY = 174
};
/* ---- Cessna172Xv2 (FB_MODEL_C172X2): fly-by-wire actuators + gain-scheduled autopilot ----------------------
 * FA/c172/c172x/c172x.jl:19-52,112-143 (Actuator1 x 7, FlyByWireActuation), c172x2.jl:18-60 (Avionics{ctl, gdc}),
 * control/c172x_ctl.jl (ControlLawsLon/Lat), FP/control.jl:123-185 (Integrator), :370-471 (PID), :620-743 (LQR),
 * :950-994 (gain lookups).
 * Continuous state x [N x FB_X2_NX], in the order of the reference's ComponentVector (`act` is the last Systems
 * field, c172.jl:678-686): rows 0-11 as Cessna172Sv0 (aero, ldg, fuel, pwp), rows FB_X2_ACT + {THROTTLE..BRAKE_RIGHT}
 * the seven actuator positions, rows 19-27 kinematics (q_wb, q_ew, h_e), rows 28-33 dynamics (w_eb_b, v_eb_b).
 * Cessna172Xv2(kinematics) (c172x2.jl:57-59) with FB_KIN_ECEF / FB_KIN_NED: the kinematic block is that mechanisation's
 * (8 rows q_eb, n_e, h_e / 6 rows psi, theta, phi, lat, lon, h_e — FP/kinematics.jl:250-425), the dynamics rows follow it
 * directly, and x has 33 / 31 rows (fb_dims reports the number).
 * Discrete state s and inputs u/ui as Cessna172Sv0, except that u's throttle/aileron/elevator/rudder (+offset) rows
 * are ignored: those four actuators are commanded by the control laws; FB_U_FLAPS / FB_U_BRAKE_* are the commands of
 * the remaining three actuators (act.flaps.u etc.). Output record y as Cessna172Sv0. */
enum {
    FB_X2_NX = 34, FB_X2_ACT = 12, FB_X2_KIN = 19, FB_X2_DYN = 28,
    FB_ACT_THROTTLE = 0, FB_ACT_AILERON = 1, FB_ACT_ELEVATOR = 2, FB_ACT_RUDDER = 3, FB_ACT_FLAPS = 4,
    FB_ACT_BRAKE_LEFT = 5, FB_ACT_BRAKE_RIGHT = 6, FB_NACT = 7
};
/* control-law inputs cu [N x FB_NCU] (avionics.ctl.u; ControlLawsLonU c172x_ctl.jl:242-253, ControlLawsLatU :826-836);
 * the two mode requests are stored as doubles holding the enum value */
enum {
    FB_CU_LON_MODE_REQ = 0, FB_CU_THROTTLE_AXIS = 1, FB_CU_THROTTLE_OFFSET = 2, FB_CU_ELEVATOR_AXIS = 3,
    FB_CU_ELEVATOR_OFFSET = 4, FB_CU_Q_REF = 5, FB_CU_THETA_REF = 6, FB_CU_EAS_REF = 7, FB_CU_CLM_REF = 8, FB_CU_H_REF = 9,
    FB_CU_LAT_MODE_REQ = 10, FB_CU_AILERON_AXIS = 11, FB_CU_AILERON_OFFSET = 12, FB_CU_RUDDER_AXIS = 13,
    FB_CU_RUDDER_OFFSET = 14, FB_CU_P_REF = 15, FB_CU_BETA_REF = 16, FB_CU_PHI_REF = 17, FB_CU_CHI_REF = 18,
    /* guidance inputs (avionics.gdc.u.mode_req, gdc.seg.u: c172x/guidance/c172x_gdc.jl:206-210, 281-283). The target segment
     * is given by its end points p1, p2 as (latitude, longitude, ellipsoidal altitude); default Segment(): (0,0,0) -> (1e-3,0,0) */
    FB_CU_GDC_MODE_REQ = 19, FB_CU_SEG_HOR_REQ = 20, FB_CU_SEG_VRT_REQ = 21, FB_CU_SEG_P1 = 22, FB_CU_SEG_P2 = 25,
    FB_NCU = 28
};
enum { FB_GDC_DIRECT = 0, FB_GDC_SEGMENT = 1, FB_GDC_CIRCULAR = 2 }; /* ModeGuidance, c172x_gdc.jl:19-23 */
enum { /* ModeControlLon, c172x_ctl.jl:29-39 */
    FB_LON_DIRECT = 0, FB_LON_SAS = 1, FB_LON_THR_Q = 2, FB_LON_THR_THETA = 3, FB_LON_THR_EAS = 4, FB_LON_EAS_Q = 5,
    FB_LON_EAS_THETA = 6, FB_LON_EAS_CLM = 7, FB_LON_EAS_ALT = 8
};
enum { FB_LAT_DIRECT = 0, FB_LAT_SAS = 1, FB_LAT_P_BETA = 2, FB_LAT_PHI_BETA = 3, FB_LAT_CHI_BETA = 4 }; /* :727-733 */
enum { FB_ALT_ACQUIRE = 0, FB_ALT_HOLD = 1 };                                                           /* :41-44 */
/* control-law record cs [N x FB_NCS]: the discrete state (s) of every compensator plus the outputs (y) other code
 * reads (modes, references, actuator commands). LQR blocks: integrator state[2], output saturation[2] (+ the last
 * z_ref[2] where a later mode change reads it); Integrator: x0, sat_out_0; PID: x_i0, x_d0, sat_out_0. */
enum {
    FB_CS_LON_MODE = 0, FB_CS_H_STATE = 1, FB_CS_THROTTLE_CMD = 2, FB_CS_ELEVATOR_CMD = 3, FB_CS_THROTTLE_REF = 4,
    FB_CS_ELEVATOR_REF = 5, FB_CS_Q_REF = 6, FB_CS_THETA_REF = 7,
    FB_CS_TE2TE = 8,    /* int[2] sat[2] z_ref[2] */
    FB_CS_TV2TE = 14,   /* int[2] sat[2] */
    FB_CS_VH2TE = 18,   /* int[2] sat[2] */
    FB_CS_Q2E_INT = 22, /* x0 sat */
    FB_CS_Q2E_PID = 24, FB_CS_C2THETA_PID = 27, FB_CS_V2T_PID = 30,
    FB_CS_LAT_MODE = 33, FB_CS_AILERON_CMD = 34, FB_CS_RUDDER_CMD = 35, FB_CS_AILERON_REF = 36, FB_CS_RUDDER_REF = 37,
    FB_CS_PHI_REF = 38,
    FB_CS_AR2AR = 39,    /* int[2] sat[2] */
    FB_CS_PHIBETA2AR = 43, /* int[2] sat[2] z_ref[2] */
    FB_CS_P2PHI_INT = 49, FB_CS_P2PHI_PID = 51, FB_CS_CHI2PHI_PID = 54,
    /* guidance outputs (gdc.y.mode, gdc.seg.y: c172x_gdc.jl:212-220, 285-289) */
    FB_CS_GDC_MODE = 57, FB_CS_SEG_DCHI = 58, FB_CS_SEG_CHI_REF = 59, FB_CS_SEG_H_REF = 60, FB_CS_SEG_HOR_GDC = 61,
    FB_CS_SEG_VRT_GDC = 62, FB_CS_SEG_E_SB = 63, FB_CS_SEG_S_1B = 64, FB_CS_SEG_S_2B = 65,
    FB_NCS = 66
};
/* FB_TABLE_CTL_GAINS blob: ten lookups in the order te2te, tv2te, vh2te (LQR, NX = 8, 8, 9), q2e, c2theta, v2t (PID),
 * ar2ar, phibeta2ar (LQR, NX = 8), p2phi, chi2phi (PID)  [files FA/c172/c172x/control/data/{te2te,tv2te,vh2te,q2e,c2θ,v2t,
 * ar2ar,φβ2ar,p2φ,χ2φ}.h5, loaded by c172x_ctl.jl:208-213,816-819]. Each lookup = 6 doubles (n_EAS, n_h, EAS_lo, EAS_hi,
 * h_lo, h_hi: the `bounds` dataset and the grid size) followed by n_EAS*n_h records, EAS index fastest. LQR record:
 * K_fbk [2 x NX] column-major, K_fwd [2 x 2], K_int [2 x 2], x_trim [NX], u_trim [2], z_trim [2]; PID record: k_p k_i k_d tau_f.
 * Interpolation: linear in (EAS, h_e), Flat extrapolation (FP/control.jl:950-966). The lookups may sit on different grids;
 * when all ten headers are equal (the reference's data files) the library locates the grid cell once per control update. */
enum { FB_CTL_GRID_HDR = 6, FB_CTL_LQR8_REC = 36, FB_CTL_LQR9_REC = 39, FB_CTL_PID_REC = 4 };

/* ---- Robot2D (FB_MODEL_ROBOT2D; FA/robot2d/robot2d.jl) ------------------------------------------------
 * state record x[FB_R2_NX]: the 4 continuous states (robot2d.jl:43) followed by the discrete state the reference
 * keeps in vehicle.u / controller.s: [w, v, theta, eta | u_m, lqr_int_out, lqr_out_sat, pid_x_i, pid_x_d, pid_sat_out]
 * inputs u[FB_R2_NU] = ControllerU (robot2d.jl:359-364): [mode (0 motor, 1 velocity, 2 position), m_ref, v_ref, eta_ref]
 * outputs y[FB_R2_NY] = VehicleY (robot2d.jl:32-41): [w, v, theta, eta, u_m, tau_m, w_dot, v_dot]; no int state (ns = 0).
 * FB_TABLE_ROBOT2D blob (23 doubles): vehicle L R m_b m_r J_b J_r k_m b_m J_m (robot2d.jl:20-30), then the
 * LQRDataPoint of robot2d.h5 K_fbk[3] K_fwd K_int x_trim[3] u_trim z_trim, then PID k_p k_i k_d tau_f (robot2d.jl:419-436). */
enum { FB_R2_NXC = 4, FB_R2_NX = 10, FB_R2_NU = 4, FB_R2_NY = 8, FB_R2_NINIT = 3, FB_R2_TABLE_SIZE = 23 };

/* ---- trim (FA/c172/c172.jl:796-818) ---- */
enum {
    FB_TP_N_E = 0, /* n_e[3] */ FB_TP_H_E = 3, FB_TP_PSI_NB = 4, FB_TP_EAS = 5, FB_TP_GAMMA_WB_N = 6,
    FB_TP_PSI_WB_DOT = 7, FB_TP_THETA_WB_DOT = 8, FB_TP_BETA_A = 9, FB_TP_FUEL_LOAD = 10, FB_TP_MIXTURE = 11,
    FB_TP_FLAPS = 12, FB_TP_PAYLOAD = 13, /* 5 masses */
    FB_NTP = 18
};
enum {
    FB_TS_ALPHA_A = 0, FB_TS_PHI_NB = 1, FB_TS_N_ENG = 2, FB_TS_THROTTLE = 3, FB_TS_AILERON = 4,
    FB_TS_ELEVATOR = 5, FB_TS_RUDDER = 6,
    FB_NTS = 7
};
/* ---- lookup tables uploaded by the host. All doubles unless noted. ---- */
enum {
    FB_TABLE_EGM96 = 0,     /* float32 [721 x 1441], column-major [lat, lon]; FP/geodesy.jl:186-198 */
    FB_TABLE_PROPELLER = 1, /* [21 x 21 x 6]: (J, Mt, {C_Fx,C_Mx,C_Fz_a,C_Mz_a,C_P,eta_p}); FP/propellers.jl:235-276 */
    FB_TABLE_PISTON = 2,    /* packed blob, layout in csrc/tables.h; FP/piston.jl:70-195 */
    FB_TABLE_AERO = 3,      /* packed blob, layout in csrc/tables.h; FA/c172/c172.jl:51-199 */
    FB_TABLE_ROBOT2D = 4,   /* FB_R2_TABLE_SIZE doubles, see above; FA/robot2d/robot2d.jl:20-30,419-436 */
    FB_TABLE_CTL_GAINS = 5, /* Cessna172Xv2 autopilot gain lookups, layout above; FP/control.jl:879-994 */
    FB_TABLE_SCENARIO = 6   /* Cessna172Xv2, Cessna172Sv0 (FB_F64): a scripted scenario as a table (below): the device-side user_callback!; FC/sim.jl:185, 334-336 */
};

/* World-level parameters shared by the whole batch (one SimpleWorld each in the reference, identical here) */
typedef struct fb_params {
    double dt;           /* integration step, FC/sim.jl:188 (default 0.02) */
    int32_t periodic_n;  /* Δt/dt ratio for f_periodic!, FC/sim.jl:189 (unused by C172Sv0: no periodic dynamics) */
    int32_t surface;     /* 0 DryTarmac, 1 WetTarmac, 2 IcyTarmac; FP/terrain.jl:13,38 */
    double T_sl, p_sl;   /* TunableSeaLevel, FP/atmosphere.jl:75-78 */
    double wind_ned[3];  /* TunableWind, FP/atmosphere.jl:165 */
    double h_terrain;    /* HorizontalTerrain elevation (orthometric), FP/terrain.jl:34-36 */
} fb_params;

/* Per-aircraft environment (optional). In the reference every simulation owns its world: TunableSeaLevel's T / p, TunableWind's
 * velocity and HorizontalTerrain's elevation are inputs / parameters of THAT world's atmosphere and terrain models
 * (FP/atmosphere.jl:75-84, 156-165, 269-278; FP/terrain.jl:34-48; FP/world.jl:20-32) — N simulations, N environments. fb_params holds ONE
 * block for the whole batch (the SURVEY's configurations share it); fb_set_env replaces its wind / sea-level / terrain-elevation
 * fields by a row per aircraft: env [N x FB_NENV] (aircraft index fastest, like every array of this ABI). The surface type stays
 * batch-wide. NULL returns to the batch-wide block. fb_trim, fb_f_ode, fb_f_step, fb_f_periodic, fb_f_init and fb_step all read the rows;
 * the stepping kernels are compiled both ways, so a handle without rows runs exactly the code it ran before (measured with rows, one
 * MI355X: Cessna172Sv0 13.92 ms per 50-step launch of 1 048 576 against 13.88, Cessna172Xv2 10.19 against 9.85 — WA mechanisation, the
 * wave-pair kernel; ECEF / NED and FB_F32 handles with rows are stepped by the one-wave fp64 kernel). Not for Robot2D (no environment). */
enum { FB_ENV_WIND_N = 0, FB_ENV_WIND_E = 1, FB_ENV_WIND_D = 2, FB_ENV_T_SL = 3, FB_ENV_P_SL = 4, FB_ENV_H_TERRAIN = 5, FB_NENV = 6 };

/* --------------------------------------------------------------------------------------------- */
/* Model(SimpleWorld(...)) + Simulation(mdl; ...) : FC/modeling.jl:103-153, FC/sim.jl:183-255.
 * device_id >= 0 selects the HIP device; there is no CPU backend (device_id < 0 is an error). */
int32_t fb_create(int32_t model_id, int32_t kin_id, int32_t dtype, int64_t n, int32_t device_id, fb_handle* out);
int32_t fb_destroy(fb_handle h);
int64_t fb_size(fb_handle h);
/* per-model array sizes: continuous+discrete real state, int state, real inputs, output record (0 where absent) */
int32_t fb_dims(fb_handle h, int32_t* nx, int32_t* ns, int32_t* nu, int32_t* ny);

/* Run on an externally created HIP stream (hipStream_t passed as void*). Every launch and copy of the handle is queued on that stream and
 * on no other: work the caller queued there before an fb_step is seen by the step, work queued behind it sees the step's result, with no
 * host synchronisation between. NULL = the handle's OWN stream (a non-blocking one it created), not HIP's null stream — a torch host whose
 * current stream is the default one (cuda_stream == 0) gets the handle's own stream and has to synchronise, or make a side stream current.
 * The call waits for everything queued on the stream the handle leaves (the caller's work on it included) before it switches; the clock,
 * the state and everything else the handle holds stay. Handles made FROM this one (fb_lss_from_linearization, fb_lss_c2d, ...) run on the
 * caller's stream it is on. The stream must outlive its use: switch back (NULL) or destroy the handle before the stream is destroyed. */
int32_t fb_set_stream(fb_handle h, void* hip_stream);
/* Use caller-owned DEVICE memory for x and s [N x FB_NS int32] (e.g. a torch tensor's data_ptr), so collectives can run
 * on the state without a host round trip. NULL, NULL restores the handle's own buffers. The buffer holds the DEVICE layout, aircraft
 * index fastest: [N x FB_NX] doubles for every Cessna172Sv0 mechanisation — rows 0-11 as in the C ABI's state; the mechanisation's
 * kinematic states from row 12 on in the C ABI's order (WA 9, ECEF 8, NED 6); then, always in rows 21-26, w_eb_b and v_eb_b — and
 * [N x FB_X2_NX] for every Cessna172Xv2 mechanisation, with the Sv0 rows first (laid out as just described: the C ABI's rows below
 * FB_X2_ACT and from FB_X2_KIN on) and the seven actuator positions (the C ABI's rows FB_X2_ACT ..) in rows 27-33. fb_get_state /
 * fb_set_state present the reference's order and row count on an attached buffer as on the handle's own.
 *   The rows a mechanisation does not use (ECEF: row 20, NED: rows 18-20) may hold anything when the buffer is attached: the call zeroes
 *   them. They are not idle — the kernels carry them through every launch and test them for finiteness with the rest — so they must stay
 *   zero afterwards; fb_set_state does not write them.
 *   Nothing is copied, by attach or by detach: after an attach the handle's state is what the caller's buffer holds (apart from the zeroed
 *   rows); after fb_attach_state(h, NULL, NULL) it is what the handle's own buffers held before the attach, which no launch has written
 *   meanwhile. The clock, the step count, the status words, the termination record, the inputs and the control-law record stay as they are.
 *   The call synchronises the handle's stream (what is queued there is done, and so is the zeroing, when it returns) and drops the derivative Cessna172Xv2 carries from one launch to
 *   the next, like every call that changes x. A caller who writes x or s in the attached buffer ITSELF (a copy, a collective, a torch
 *   kernel) announces that by calling fb_attach_state again with the same pointers, before the next fb_step; without the call a
 *   Cessna172Xv2 may step from the derivative of the state it had.
 *   x_dev must be 8-byte aligned and s_dev 4-byte aligned (a view into a larger tensor is fine: every access is one element wide); x
 *   without s, s without x, a misaligned pointer, a Robot2D or a LinearizedSS handle are refused, and a refusal changes nothing. */
int32_t fb_attach_state(fb_handle h, void* x_dev, void* s_dev);

/* Lookup tables: what the reference builds at construction time (Appendix B of SURVEY.md). */
int32_t fb_set_table(fb_handle h, int32_t kind, const void* data, const int64_t* dims, int32_t ndims);
int32_t fb_set_params(fb_handle h, const fb_params* p);
int32_t fb_get_params(fb_handle h, fb_params* p);
/* world.atmosphere.{sl, wind}.u / terrain elevation, one row per aircraft (see FB_ENV_* above); env = NULL: back to fb_params.
 * fb_get_env fails when no rows are set. */
int32_t fb_set_env(fb_handle h, const double* env);
int32_t fb_get_env(fb_handle h, double* env);
int32_t fb_has_env(fb_handle h);   /* 1: per-aircraft rows are set, 0: the batch-wide block is in force, < 0: error */

/* mdl.x / mdl.s / mdl.u access : FC/modeling.jl:89-101 ; property forwarding FC/sim.jl:261-275.
 * fb_set_state sets an INITIAL condition: like init! (FC/sim.jl:390-414) it also clears the sticky status words and restarts the
 * clock and the phase of the periodic update. fb_assign_state is the plain `mdl.x .= v` / `mdl.s = v` of a user callback in the
 * middle of a run (FC/sim.jl:331-341): t, the step count and the status words stay as they are. */
int32_t fb_set_state(fb_handle h, const double* x, const int32_t* s);
int32_t fb_assign_state(fb_handle h, const double* x, const int32_t* s);
int32_t fb_get_state(fb_handle h, double* x, int32_t* s);
int32_t fb_set_inputs(fb_handle h, const double* u, const int32_t* ui);
int32_t fb_get_inputs(fb_handle h, double* u, int32_t* ui);

/* f_init!(world, C172.TrimParameters): FP/world.jl:49-57 -> FA/c172/c172.jl:883-942.
 * trim_params [N x FB_NTP]; trim_state [N x FB_NTS] in: initial guess (c172.jl:796-804), out: solution.
 * success[i] = 1 when cost <= 1e-16 (the reference's STOPVAL_REACHED criterion, c172.jl:926,934).
 * On return x, s, u hold the trimmed initial condition (assign!, FA/c172/c172s/c172s.jl:227-263). */
int32_t fb_trim(fb_handle h, const double* trim_params, double* trim_state, int32_t* success, double* cost);

/* f_init!(mdl, init) with a plain per-instance initializer: Robot2D InitParameters [N x 3] = (u_m, w, eta),
 * FA/robot2d/robot2d.jl:208-228,563-570. (C172 initialises through fb_trim or fb_set_state.)
 * Cessna172Xv2 with init = NULL, ninit = 0: the avionics half of f_init!(aircraft, C172.Init(...)) (aircraftbase.jl:255-265) on the
 * state already set with fb_set_state / fb_set_inputs — actuator states = the commands in u (c172x.jl:253-271), brakes released,
 * then f_init!(avionics, vehicle). */
int32_t fb_f_init(fb_handle h, const double* init, int32_t ninit);

/* ---- linearize (FP/linearization.jl:55-148, FP/aircraftbase.jl:292-334, FA/robot2d/robot2d.jl:233-341) ---------------------------
 * The state-space vectors x_ss / u_ss / y_ss of get_x_ss / get_u_ss / get_y_ss: Cessna172Sv0(NED) 16 / 4 / 33 (FA/c172/c172s/c172s.jl:269-412),
 * Cessna172Xv2(NED) 20 / 4 / 38 (its vehicle, FA/c172/c172x/c172x.jl:332-490: u_ss = the four actuator COMMANDS, substituted where the
 * actuators read them; avionics take no part), Robot2D 4 / 1 / 6 (robot2d.jl:233-275). WA / ECEF Cessnas and FB_F32 handles have none.
 * Outputs in the ABI's convention, aircraft index fastest: xdot0, x0 [N x nx], u0 [N x nu], y0 [N x ny]; the matrices column-major per
 * aircraft: element (i, r, c) of A [N x nx x nx] at A[(r + nx c) N + i], B [N x nx x nu], C [N x ny x nx], D [N x ny x nu]. Every output
 * pointer may be NULL (a NULL block is not copied; with A, B or C, D both NULL that half is not written on the device either).
 * lin_status[i] = the OR of the FB_ST_* bits of every evaluation of aircraft i (where the reference would throw out of linearize).
 * Schemes: FB_LIN_FORWARD = FiniteDiff's default forward Jacobian, the reference's: step max(2^-26 |z|, 2^-26), (f(z + e) - f(z)) / e,
 * 1 + nx + nu evaluations per aircraft; FB_LIN_ONESIDED2 = (-3 f(z) + 4 f(z + h) - f(z + 2h)) / 2h with h = (z + 1e-6 max(|z|, 1)) - z,
 * 1 + 2 (nx + nu) evaluations, ~1e-10 instead of ~1e-8 (docs/design/linearize.md). Host copy of a full result: 8 x (2 nx + nu + ny +
 * (nx + ny)(nx + nu)) bytes per aircraft (Cessna172Sv0: 8.4 KB). */
enum { FB_LIN_FORWARD = 0, FB_LIN_ONESIDED2 = 1 };
/* nx, nu, ny of get_x_ss / get_u_ss / get_y_ss for this handle's vehicle (refuses handles that have none) */
int32_t fb_linearize_dims(fb_handle h, int32_t* nx, int32_t* nu, int32_t* ny);
/* linearize(vehicle, trim_params): FP/aircraftbase.jl:292-334, FA/robot2d/robot2d.jl:315-341.
 * Cessna: params = trim parameters [N x FB_NTP], trim_state [N x FB_NTS] in/out, success / cost as fb_trim. The trim runs in the reference's
 * own environment — ISA sea level, no wind, terrain elevation 0, DryTarmac — whatever fb_set_params / fb_set_env say (those stay in place,
 * unused by this call); the handle is left as fb_trim leaves it after a still-air trim (x, s, u, Cessna172Xv2's control laws, clock,
 * status words, termination record). Robot2D: params = InitParameters [N x 3] (NULL: the defaults), trim_state / success / cost unused;
 * the handle is left as fb_f_init leaves it. */
int32_t fb_linearize(fb_handle h, const double* params, double* trim_state, int32_t* success, double* cost, int32_t scheme,
                     double* xdot0, double* x0, double* u0, double* y0, double* A, double* B, double* C, double* D, int32_t* lin_status);
/* linearize(f, h, x0, u0) at the handle's CURRENT x, u, s (Cessna172Xv2: the commands in its control-law record) and environment
 * (fb_params block or fb_set_env rows, as fb_f_ode): FP/linearization.jl:55-111. Changes nothing on the handle. */
int32_t fb_linearize_state(fb_handle h, int32_t scheme, double* xdot0, double* x0, double* u0, double* y0,
                           double* A, double* B, double* C, double* D, int32_t* lin_status);

/* ---- Model(lss): LinearizedSS as a model (FB_MODEL_LSS; FP/linearization.jl:157-192) -------------------------------------------------
 * A batch of N linear systems xdot = xdot0 + A (x - x0) + B (u - u0), y = y0 + C (x - x0) + D (u - u0), each with its own matrices, all
 * with one (nx, nu, ny): 1 <= nx <= 32, 1 <= nu <= 8, 1 <= ny <= 64 (Robot2D 4 / 1 / 6, Cessna172Sv0 16 / 4 / 33, Cessna172Xv2 20 / 4 / 38 and
 * every subsystem of them); FB_F64 only. The generic verbs serve such a handle: fb_size, fb_dims (Ns = 0), fb_set_state / fb_assign_state /
 * fb_get_state (x [N x nx], s unused), fb_set_inputs / fb_get_inputs (u [N x nu], ui NULL), fb_f_ode (xdot [N x nx] and the record),
 * fb_get_outputs (y [N x ny]), fb_step (RK4, u held over the call), fb_set_steps_per_launch, fb_set_params / fb_get_params (dt; the
 * rest is unused), fb_time, fb_sync, fb_set_stream, fb_status (a linear model throws nothing: zeros), fb_get_step_count /
 * fb_set_step_count, fb_timing_*, fb_log_* (output rows [0, ny), FB_LOG_X0 + state row), fb_destroy. fb_f_step and fb_f_periodic return 0
 * and do nothing (@no_step, @no_periodic, :161-162). Verbs of other model families (trim, environment, tables, control laws, scenarios,
 * linearize, RCCL gather, attach) fail with a message that names LinearizedSS. */
/* Model(lss) for N systems of dimensions (nx, nu, ny) on device_id; the model comes from fb_lss_set_model. FC/modeling.jl:103-153 */
int32_t fb_lss_create(int32_t nx, int32_t nu, int32_t ny, int64_t n, int32_t device_id, fb_handle* out);
/* the LinearizedSS of every system (FP/linearization.jl:39-48), host arrays in exactly the layout fb_linearize writes them. Leaves
 * x = x0 and u = u0 (Modeling.X(lss) = copy(lss.x0), Modeling.U(lss) = copy(lss.u0), :157-158), t = 0 and the step count 0. */
int32_t fb_lss_set_model(fb_handle h, const double* xdot0, const double* x0, const double* u0, const double* y0,
                         const double* A, const double* B, const double* C, const double* D);
/* Model(subsystem(lss; x, u, y)) (FP/linearization.jl:113-132) device to device: lss = the result of src's last fb_linearize or
 * fb_linearize_state, which is still on src's device (every block must have been requested in that call); ix [nx], iu [nu], iy [ny] = the rows
 * and columns to keep, in the order given (NULL: every index in order, the count argument is then ignored). The new handle is on src's
 * device (and on src's stream when that is the caller's own), takes src's dt, and starts at x = x0, u = u0, t = 0. */
int32_t fb_lss_from_linearization(fb_handle src, const int32_t* ix, int32_t nx, const int32_t* iu, int32_t nu,
                                  const int32_t* iy, int32_t ny, fb_handle* out);
/* how the handle's stepper exchanges the stage values inside a group of lanes: *xch = 0 the LDS panel (the default), 1 cross-lane reads
 * (FLIGHTBATCH_LSS_EXCHANGE=shfl in the environment when the handle was created; the two give the same bits: docs/design/linearize.md).
 * Works before a model is set; changes nothing on the handle. */
int32_t fb_lss_exchange(fb_handle h, int32_t* xch);
/* the handle's own copy of the model, as its kernels read it: A [nx x nx] and B [nx x nu] of every system, host arrays in fb_linearize's
 * layout (either may be NULL). Changes nothing on the handle. */
int32_t fb_lss_get_model(fb_handle h, double* A, double* B);

/* ---- lqr(P, Q, R) on a Model(lss) batch (FA design scripts: design/c172/c172x_design.jl:181 `lqr(P, Q, R)`, also :369, :475, :588, :651;
 * design/robot2d/robot2d_design.jl:58) -------------------------------------------------------------------------------------------------
 * For every system of an FB_MODEL_LSS handle with 1 <= nx <= FB_LQR_NX_MAX: the stabilising solution X of A'X + XA - X B inv(R) B' X + Q = 0 and
 * the gain K = inv(R) B' X, by the matrix sign function of the Hamiltonian (Newton's iteration with determinant scaling, at most 50
 * iterations; docs/design/linearize.md, "LQR design on the device"). Q [nx x nx] and R [nu x nu] are column-major host arrays, one pair for
 * the batch: both symmetric (compared exactly), R positive definite. Outputs are host arrays, any may be NULL: element (i, r, c) of
 * K [nu x nx] at K[(r + nu c) N + i], of X [nx x nx] at X[(r + nx c) N + i] (fb_linearize's layout); resid [N] = max|A'X + XA - XGX + Q| /
 * max(max|Q|, max|X|); iters [N] = Newton iterations taken; status [N] = 0 or FB_LQR_* bits. A system with a non-zero status has K, X and
 * resid = NaN; the call still returns 0. Reads A and B from the handle's copy of the model and changes nothing on the handle. */
enum { FB_LQR_NOT_CONVERGED = 1,   /* the iteration bound was reached (eigenvalues of the Hamiltonian on or near the imaginary axis) */
       FB_LQR_SINGULAR = 2,        /* a zero or non-finite pivot, or a non-finite result: no stabilising solution */
       FB_LQR_NX_MAX = 16 };
int32_t fb_lqr(fb_handle lss, const double* Q, const double* R, double* K, double* X, double* resid, int32_t* iters, int32_t* status);

/* ---- the metrics of optimize_PID on a Model(lss) batch (FA design/pidopt.jl: build_PID :31-34, Metrics :36-64, cost :66-70, evaluated by
 * optimize_PID :73-128 at every node of design/c172/c172x_design.jl, e.g. :236 for q2e; docs/design/linearize.md, "PID loop design on the
 * device") ---------------------------------------------------------------------------------------------------------------------------
 * The plant is channel (iu, iy) of each system of an FB_MODEL_LSS handle with 1 <= nx <= FB_PID_NX_MAX, in deviation coordinates: A,
 * b = B[:, iu], c = C[iy, :], d = D[iy, iu] (xdot0, x0, u0, y0 play no part). Both calls read the handle's copy of the model, run on its
 * stream and change nothing on the handle. w [nw]: 1 <= nw <= 1024 frequencies in rad/s, all positive and finite.
 * fb_lss_freqresp: P(j w) = c inv(j w I - A) b + d (the plant of sensitivity(plant, pid), pidopt.jl:39) by complex Gauss-Jordan elimination
 * with row pivoting; re, im [nw x N], system index fastest: element (k, i) at [k N + i]; NaN where a pivot was zero or not finite. */
int32_t fb_lss_freqresp(fb_handle lss, int32_t iu, int32_t iy, const double* w, int32_t nw, double* re, double* im);
/* fb_pid_metrics: Metrics(plant, pid, settings) and cost (pidopt.jl:36-70) of m candidates per system, 1 <= m <= 64. pid [4 x m x N]:
 * (k_p, k_i, k_d, tau_f) of candidate j of system i at pid[(f m + j) N + i], tau_f > 0; C(s) = k_p + k_i / s + k_d s / (tau_f s + 1)
 * (build_PID :31-34). Unit step of the reference from rest over N_t = round(t_sim / dt) <= 200000 steps of the classical RK4 (dt > 0,
 * t_sim >= dt), sampled at t_k = k dt. metrics [5 x m x N] (may be NULL), row order Ms, ie, ef, iu, up (Metrics :8-14): Ms = min(1e3, max over
 * the grid of |1 / (1 + P C)|) (:39-43), ie = trapz|y - 1| / t_N, ef = |y_N - 1| (:45-52), iu = trapz|u - 1| / t_N, up = max|u - 1| (:54-60,
 * the reference's expression). cost [m x N] = sum weights m / sum weights (:66-70); weights [5] >= 0 with a positive sum, NULL = ones.
 * status [m x N]: 0; FB_PID_DIVERGED: a sample was not finite or beyond 1e12 (ie, ef, iu, up and cost are +Inf, Ms is the grid's);
 * FB_PID_SINGULAR: a zero or non-finite pivot at some frequency, or 1 + d (k_p + k_d / tau_f) = 0 (the metrics are NaN, cost is +Inf).
 * The call returns 0 in both cases. Not the reference's: its step() picks the sample time and discretises exactly (here: fb_lss_c2d, which
 * this verb does not use yet), and its hinfnorm2 finds the exact peak and is infinite for an unstable loop. */
enum { FB_PID_DIVERGED = 1, FB_PID_SINGULAR = 2, FB_PID_NX_MAX = 28 };
int32_t fb_pid_metrics(fb_handle lss, int32_t iu, int32_t iy, const double* w, int32_t nw, double t_sim, double dt, const double* weights,
                       const double* pid, int32_t m, double* metrics, double* cost, int32_t* status);

/* ---- the poles of a Model(lss) batch (FA design/robot2d/robot2d_design.ipynb: `dampreport(P)` on the open loop and on the LQR velocity
 * loop; docs/design/linearize.md, "Poles on the device") ---------------------------------------------------------------------------------
 * For every system of an FB_MODEL_LSS handle (1 <= nx <= FB_POLES_NX_MAX, all that fb_lss_create admits): the nx eigenvalues of A by the
 * classical dense path, eigenvalues only: balancing by powers of two without permutation, Householder reduction to Hessenberg form,
 * double-shift QR with deflation (at most 30 sweeps per window, exceptional shifts at sweeps 10 and 20). Outputs are host arrays, any may be
 * NULL: re, im [nx x N], system index fastest: element (k, i) at [k N + i]; iters [N] = QR sweeps taken; status [N] = 0 or FB_POLES_* bits.
 * Within a system the poles ascend by |pole|, then Re, then Im, then the position the elimination left them in (dampreport's order by
 * natural frequency: a function of the system's own values only); a complex pair is stored as exact conjugates, the same Re bits and
 * +-Im. A system with a non-zero status has NaN poles; the call still returns 0. Reads A from the handle's copy of the model, runs on its
 * stream and changes nothing on the handle. */
enum { FB_POLES_NOT_CONVERGED = 1,   /* a window took 30 sweeps without deflating */
       FB_POLES_NOT_FINITE = 2,      /* a non-finite entry in A (the system is not iterated on: iters = 0), or a non-finite result */
       FB_POLES_NX_MAX = 32 };
int32_t fb_lss_poles(fb_handle lss, double* re, double* im, int32_t* iters, int32_t* status);

/* ---- step responses and StepInfo of a Model(lss) batch (FA design/robot2d/robot2d_design.ipynb: `step(P[:y, :u], t_sim)` and `stepinfo` of
 * it on the velocity loop and on the position loop; docs/design/linearize.md, "Step responses on the device") -------------------------------
 * For m channels (iu[j], iy[j]), 1 <= m <= 64, of every system of an FB_MODEL_LSS handle with 1 <= nx <= FB_STEPINFO_NX_MAX: the unit step
 * response of x' = A x + b, y = c x + d (b = B[:, iu], c = C[iy, :], d = D[iy, iu]; xdot0, x0, u0, y0 play no part) from rest, sampled at
 * t_k = k dt, k = 0 .. N_t, N_t = round(t_sim / dt) <= 200000, by the classical RK4 (dt > 0, t_sim >= dt). Pair (j, i) of channel j and
 * system i is stored at [j N + i], the system index fastest.
 * opts: NULL or {settling_th, rise_lo, rise_hi} (NULL = 0.02, 0.1, 0.9; settling_th > 0, 0 < rise_lo < rise_hi < 1).
 * y0_in, yf_in: NULL or [m x N], the initial and final value stepinfo measures from; a NaN entry (and NULL) means the first / last sample.
 * y: NULL or [ns x m x N], ns = fb_lss_stepinfo_samples(N_t, stride) = ceil(N_t / stride) + 1: sample s stride at row s, and sample N_t at
 * the last row whether stride divides N_t or not (stride >= 1).
 * info [9 x m x N], row order y0, yf, stepsize, peak, peaktime, overshoot, undershoot, settlingtime, risetime: stepsize = |yf - y0|,
 * dir = sign(yf - y0); peak = max y (dir > 0) or min y (dir < 0) at its first index, peaktime that index times dt; overshoot =
 * dir 100 (peak - yf) / stepsize; undershoot = 100 (y0 - min y) / stepsize for dir > 0, 100 (max y - y0) / stepsize for dir < 0, not below 0;
 * settlingtime = t one sample past the last sample with |y - yf| > settling_th stepsize, at most t_N, 0 if there is none; risetime =
 * t[first k with dir (y_k - y0) > rise_hi stepsize] - t[first k with dir (y_k - y0) > rise_lo stepsize], NaN if either is never reached.
 * status [m x N]: 0; FB_STEPINFO_DIVERGED: a sample was not finite or beyond 1e12 (every info row is NaN); FB_STEPINFO_FLAT: stepsize is 0
 * or not finite (y0, yf, stepsize, peak and peaktime as defined with dir = +1; the four ratios and times are NaN). The call returns 0 in both
 * cases. Reads the handle's copy of the model, runs on its stream and changes nothing on the handle. Not the reference's: its step() picks
 * the sample time and discretises exactly; the exact samples at the caller's dt are those of the same call on the handle fb_lss_c2d makes
 * (below), which samples the map instead of integrating. */
enum { FB_STEPINFO_DIVERGED = 1, FB_STEPINFO_FLAT = 2, FB_STEPINFO_NX_MAX = 31 };
int32_t fb_lss_stepinfo_samples(int32_t nsteps, int32_t stride);   /* -1 unless nsteps >= 1 and stride >= 1 */
int32_t fb_lss_stepinfo(fb_handle lss, const int32_t* iu, const int32_t* iy, int32_t m, double t_sim, double dt, const double* opts,
                        const double* y0_in, const double* yf_in, int32_t stride, double* y, double* info, int32_t* status);

/* ---- connect / series / feedback on Model(lss) batches (FA design/c172/c172x_design.jl:199-216, 226-227, 244-263, ...: the `connect`,
 * `series` and `feedback` calls between the design verbs; docs/design/linearize.md, "Closing loops on the device") --------------------------
 * The plant p (nx_p, nu_p, ny_p) and the optional compensator c (nx_c, nu_c, ny_c; NULL: none), two FB_MODEL_LSS handles with the same N on
 * one device, are connected through static gains into a new FB_MODEL_LSS handle, system by system, in deviation coordinates (the offsets
 * xdot0, x0, u0, y0 play no part, as named_ss(lss) drops them). With v = [u_p; u_c] (nv rows), z = [y_p; y_c] (nz rows), x = [x_p; x_c] and
 * the block-diagonal stacked model x' = A x + B v, z = C x + D v:
 *     v = F z[jz] + G w           jz [nf]: the rows of z the feedback reads; F [nv x nf]; w: the nw inputs of the new model; G [nv x nw]
 *     E = inv(I - F D[jz, :]), M = E F C[jz, :], Nw = E G
 *     A' = A + B M,  B' = B Nw,  C' = C[iz, :] + D[iz, :] M,  D' = D[iz, :] Nw          iz [ny]: the rows of z the new model outputs
 * F and G are host arrays, column-major: one matrix for the batch (*_per_system = 0) or one per system in fb_linearize's layout, element
 * (i, r, col) at [(r + rows col) N + i] (K of fb_lqr is in that layout). iz = NULL means every row of z (nz <= 64). status [N] may be NULL:
 * 0; FB_CONNECT_NOT_FINITE: a non-finite entry in the source models, in F or in G; otherwise FB_CONNECT_ILL_POSED: a zero or non-finite
 * pivot of I - F D[jz, :] (Gauss-Jordan elimination, the pivot of a step the largest magnitude among the rows not yet used). Such a system
 * gets A', B', C', D' all NaN; the call still returns 0 and no other system changes in any bit.
 * The new handle: on p's device, with p's dt and p's stream rule (fb_lss_from_linearization), at x = 0, u = 0, t = 0, xdot0 = x0 = u0 = y0 =
 * 0; every verb of an FB_MODEL_LSS handle works on it. p and c are only read. Refused, with nothing launched and no handle created: a NULL or
 * non-LSS p, a non-LSS c, a handle without a model, c on another device or with another N, nx_p + nx_c > 32, nv > FB_CONNECT_NV_MAX,
 * nz > FB_CONNECT_NZ_MAX, nf outside 1 .. FB_CONNECT_NF_MAX, nw outside 1 .. 8, ny outside 1 .. 64, an index of jz or iz outside [0, nz),
 * NULL F, G, jz or out. */
enum { FB_CONNECT_ILL_POSED = 1, FB_CONNECT_NOT_FINITE = 2, FB_CONNECT_NV_MAX = 16, FB_CONNECT_NF_MAX = 32, FB_CONNECT_NZ_MAX = 128 };
int32_t fb_lss_connect(fb_handle p, fb_handle c /* NULL: no compensator */, const int32_t* jz, int32_t nf, const double* F, int32_t f_per_system,
                       const double* G, int32_t g_per_system, int32_t nw, const int32_t* iz, int32_t ny, int32_t* status, fb_handle* out);
/* The companion of fb_lss_get_model: C [ny x nx x N] and D [ny x nu x N] of the handle's own copy, in fb_linearize's layout (either may be NULL). */
int32_t fb_lss_get_cd(fb_handle h, double* C, double* D);

/* ---- design-model surgery on Model(lss) batches (FA design/c172/c172x_design.jl:23-82: get_design_model!, subsystem, delete_vars; :184-188,
 * :371-381: K_fwd; docs/design/linearize.md, "Design-model surgery on the device") ---------------------------------------------------------
 * fb_lss_transform: a change of state variables, then a subsystem, of every model of an FB_MODEL_LSS handle into a new FB_MODEL_LSS handle.
 * rows [nx] names output rows of the source; with T = C[rows, :]
 *     A' = T A inv(T),  B' = T B,  C' = C inv(T),  D' = D,  x0' = y0[rows],  xdot0' = T xdot0,  u0 and y0 as they are
 * and the entries r of xdot0' with xdot_zero[r] != 0 are exactly 0 (xdot_zero [nx] may be NULL: none). D[rows, :] is ignored, as the
 * reference ignores it: the new states are the outputs y[rows] only where those rows of D are zero. Then the lists ix [nxo], iu [nuo],
 * iy [nyo] select states, inputs and outputs of the transformed model, in the order given (NULL: all of them, the count is ignored). With
 * rows == NULL, T is the identity and no arithmetic is done: the new handle's entries are copies, bit for bit (subsystem device to device).
 * status [N] and rpiv [N] may be NULL. status: 0; FB_SURGERY_NOT_FINITE: a non-finite entry of the source's A, B, C, D or xdot0; otherwise
 * FB_SURGERY_SINGULAR: a zero or non-finite pivot of T (Gauss-Jordan elimination, the pivot of a step the largest magnitude among the rows
 * not yet used). Such a system gets A', B', C', D' and xdot0' all NaN; the call still returns 0 and no other system changes in any bit.
 * rpiv: the smallest pivot magnitude over the largest (1 with rows == NULL; 0 for a singular system, NaN for a non-finite one), the
 * warning of a nearly singular T. The new handle: on the source's device, with its dt and its stream rule (fb_lss_from_linearization), at
 * x = x0', u = u0, t = 0. The source is only read. Refused, with nothing launched and no handle created: a NULL or non-LSS handle, a handle
 * without a model, an index of rows outside [0, ny), of ix outside [0, nx), of iu outside [0, nu), of iy outside [0, ny), nxo, nuo or nyo
 * below 1 or above the source's size, a NULL out.
 * fb_lss_steady: the steady-state map of every model. iz [nz] names output rows, nz == nu; with L = [A B; C[iz, :] D[iz, :]]
 *     L [X; U] = [0; I],  K_fwd = U + K X          X [nx x nz] = M12 and U [nu x nz] = M22 of M = inv(L)
 * K [nu x nx] is a host array, column-major: one matrix for the batch (k_per_system = 0) or one per system in fb_linearize's layout (fb_lqr's
 * K); NULL: no K_fwd (K_fwd must be NULL as well). X, U, K_fwd come home in fb_linearize's layout, element (i, r, c) at [(r + rows c) N + i];
 * each of them, rpiv [N] and status [N] may be NULL. status and rpiv as above, for L (NOT_FINITE: an entry of L or of K); X, U, K_fwd of such
 * a system are NaN. Refused: a NULL or non-LSS handle, a handle without a model, nx + nu > FB_SURGERY_N_MAX, nz != nu, a NULL iz, an index
 * of iz outside [0, ny), K_fwd without K. */
enum { FB_SURGERY_SINGULAR = 1, FB_SURGERY_NOT_FINITE = 2, FB_SURGERY_N_MAX = 32 };
int32_t fb_lss_transform(fb_handle lss, const int32_t* rows, const int32_t* xdot_zero, const int32_t* ix, int32_t nxo, const int32_t* iu, int32_t nuo,
                         const int32_t* iy, int32_t nyo, int32_t* status, double* rpiv, fb_handle* out);
int32_t fb_lss_steady(fb_handle lss, const int32_t* iz, int32_t nz, const double* K, int32_t k_per_system, double* X, double* U, double* K_fwd,
                      double* rpiv, int32_t* status);

/* ---- sampled models: zero-order-hold discretisation on the device (the exact samples of ControlSystems' step and lsim, FA design/pidopt.jl,
 * demos/c172_demos.jl:135, 186; docs/design/linearize.md, "Sampled models on the device") ---------------------------------------------------
 * fb_lss_c2d: for every system of a continuous FB_MODEL_LSS handle (1 <= nx <= 32, every nu and ny the handle admits), with
 *     Psi = int_0^Ts e^(A tau) dtau:   Phi = e^(A Ts) = I + A Psi,  Gamma = Psi B,  delta = Psi xdot0
 * a new FB_MODEL_LSS handle of the same N, nx, nu, ny whose copy of the model holds Phi in A's place, Gamma in B's and delta in xdot0's; C, D,
 * x0, u0 and y0 are copied bit for bit. The affine offset is carried exactly: x+ = x0 + Phi (x - x0) + Gamma (u - u0) + delta. The new handle
 * is marked sampled with sample time Ts: its dt is Ts, x = x0, u = u0, t = 0; on the source's device, with its stream rule
 * (fb_lss_from_linearization). The source is only read. By scaling and squaring of the pair (Phi, Psi [B | xdot0]) with s = the smallest
 * integer >= 0 with |A|_inf Ts / 2^s <= 1/2; A is never inverted (a singular A, an integrator in series, is an ordinary input).
 * squarings [N] and status [N] may be NULL. status: 0; FB_C2D_NOT_FINITE: a non-finite entry of A, B or xdot0, or a non-finite result (an
 * overflowing e^(A Ts)); FB_C2D_RANGE: s would exceed FB_C2D_SQUARINGS_MAX. Such a system gets Phi, Gamma and delta all NaN; the call still
 * returns 0 and no other system changes in any bit. squarings: s (0 where there is a status). Refused, with nothing launched and no handle
 * created: a NULL or non-LSS handle, a handle without a model, a handle that is itself sampled, Ts not finite or <= 0, a NULL out.
 * fb_lss_sample_time: Ts of a sampled handle, 0 for a continuous LinearizedSS handle.
 * A sampled handle under the other verbs: fb_step applies the map (one step = Ts on the clock; refused once fb_set_params has made dt differ
 * from Ts in any bit); fb_f_ode(NULL) refreshes y, fb_f_ode(xdot) is refused (no derivative); fb_lss_get_model returns Phi and Gamma;
 * fb_lss_get_cd is unchanged; fb_lss_stepinfo samples the map at t_k = k Ts (dt must be Ts bit for bit; 0 or a non-finite dt means Ts);
 * fb_lss_set_model, fb_lss_c2d, fb_lqr, fb_pid_metrics, fb_lss_freqresp, fb_lss_poles, fb_lss_connect (either argument),
 * fb_lss_transform and fb_lss_steady are refused ("a continuous-time verb on a sampled model"); fb_lss_dlqr (below) designs on it, and
 * fb_lss_dsteady (below) is the steady-state map of a sampled model. */
enum { FB_C2D_NOT_FINITE = 1, FB_C2D_RANGE = 2, FB_C2D_SQUARINGS_MAX = 30 };
int32_t fb_lss_c2d(fb_handle lss, double Ts, int32_t* squarings /* [N] or NULL */, int32_t* status /* [N] or NULL */, fb_handle* out);
int32_t fb_lss_sample_time(fb_handle h, double* Ts);   /* 0 for a continuous LinearizedSS handle */

/* ---- the discrete LQR of a batch of sampled models (ControlSystems' lqr(Discrete, Phi, Gamma, Q, R), the sampled-data counterpart of the
 * design scripts' lqr(P, Q, R); the controllers of FP/control.jl run in f_periodic! at dt = 0.02; docs/design/linearize.md, "Discrete LQR on
 * the device") ----------------------------------------------------------------------------------------------------------------------------
 * For every system of a SAMPLED FB_MODEL_LSS handle (fb_lss_c2d) with 1 <= nx <= FB_DLQR_NX_MAX and 1 <= nu <= 8, Phi and Gamma read from
 * the handle's copy of the model: the stabilising solution X of
 *     X = Phi' X Phi - Phi' X Gamma inv(R + Gamma' X Gamma) Gamma' X Phi + Q
 * and the gain K = inv(R + Gamma' X Gamma) Gamma' X Phi (u = u0 - K (x - x0)), by the structure-preserving doubling algorithm on
 * (A, G, H) = (Phi, Gamma inv(R) Gamma', Q): W = I + G H, [V | U] = inv(W) [A | G], H <- H + A' (H V), G <- G + (A U) A', A <- A V, until
 * max|dH| <= 1e-13 max|H| and max|A| <= 2^-20 (A_k is the closed loop over 2^k samples), at most FB_DLQR_MAX_ITERS doublings; X = (H + H') / 2,
 * K = inv(R) Gamma' X inv(I + G0 X) Phi. Phi is never inverted (an eigenvalue at 0 is an ordinary input). Q, R and the outputs K, X, iters
 * and status follow fb_lqr's conventions exactly (one pair of column-major host weights for the batch, symmetry compared exactly, R positive
 * definite, Q finite; fb_linearize's layout; any output may be NULL). resid [N] = max|Phi' X Phi - X - Phi' X Gamma K + Q| / max(max|Q|,
 * max|X|); iters [N] = the doublings taken. status [N]: 0; FB_DLQR_NOT_CONVERGED: the bound was reached (a mode on the unit circle that the
 * weights do not see, or one that no input reaches); FB_DLQR_SINGULAR: a zero or non-finite pivot, or a non-finite A, G, H, K or residual.
 * A system with a status has K, X and resid = NaN; the call still returns 0 and no other system changes in any bit.
 * closed (may be NULL: then nothing is allocated): a new sampled FB_MODEL_LSS handle of the same N, nx, nu, ny and Ts that holds the designed
 * loop with input v, u = v - K (x - x0): Phi - Gamma K in A's place, C - D K in C's; Gamma, D, delta, x0, u0 and y0 copied bit for bit; at
 * x = x0, u = u0, t = 0; on the source's device, with its stream rule. A system with a status gets Phi - Gamma K and C - D K all NaN.
 * The source is only read. Refused, with nothing launched and no handle created: a NULL or non-LSS handle, a handle without a model, a
 * continuous handle (fb_lss_c2d is the way in), nx > FB_DLQR_NX_MAX, a NULL, asymmetric or non-finite Q, a NULL or asymmetric R or one that
 * is not positive definite. */
enum { FB_DLQR_NOT_CONVERGED = 1, FB_DLQR_SINGULAR = 2, FB_DLQR_MAX_ITERS = 40, FB_DLQR_NX_MAX = 16 };
int32_t fb_lss_dlqr(fb_handle lss, const double* Q, const double* R, double* K, double* X, double* resid, int32_t* iters, int32_t* status,
                    fb_handle* closed /* or NULL */);

/* ---- gain and phase margins of a batch of loops (FA design/robot2d/robot2d_design.ipynb: `marginplot(P_v[:η, :v_ref])` and
 * `marginplot(series(C_η2v, P_v2η))`; docs/design/linearize.md, "Margins on the device") -----------------------------------------------------
 * The loop of system i is L_i(jw) = gain_i (c inv(jw I - A) b + d) of channel (iu, iy) of a continuous FB_MODEL_LSS handle with a model and
 * 1 <= nx <= FB_MARGINS_NX_MAX, in deviation coordinates, under negative unity feedback (the closed loop is 1 + L). gain [N] or NULL (ones).
 * w [nw]: 2 <= nw <= 1024 frequencies in rad/s, positive, finite and strictly increasing. With L_k = L(j w_k), interval k brackets
 *   a phase crossing when (Im L_k < 0) != (Im L_k+1 < 0), unless Re L >= 0 at both ends (a crossing of the positive real axis);
 *   a gain crossing when (|L_k|^2 < 1) != (|L_k+1|^2 < 1).
 * Every bracket is refined by geometric bisection on its own predicate: mid = sqrt(lo hi); stop when mid is not strictly inside (lo, hi) or
 * after 60 halvings; lo = mid when the predicate at mid equals the one at lo, else hi = mid. The crossing is w* = the final lo, L* = L(j w*).
 * A refined phase bracket counts when Re L* < 0 (gm = -1 / Re L*), a refined gain bracket always (pm = atan2(-Im L*, -Re L*) in degrees, in
 * (-180, 180]). At most FB_MARGINS_KMAX crossings of a kind are kept, in ascending frequency; one more sets FB_MARGINS_TRUNCATED and the
 * count stays at FB_MARGINS_KMAX. Selected: the kept phase crossing with the smallest max(g, 1 / g), g = -Re L* (the gain margin closest to
 * 1 in either direction), and the kept gain crossing with the largest -Re L* / |L*| (the smallest |pm|); ties go to the lower frequency.
 * The device selects by comparing products; gm, pm and the square root of smin are computed by the host side of this call.
 * sel [10 x N], row order gm, wpc, pm, wgc, Re L* and Im L* at the phase crossing, Re L* and Im L* at the gain crossing, smin = the minimum
 * over the grid of |1 + L_k| (the grid's value, as fb_pid_metrics' Ms is: Ms = 1 / smin), wsmin = the grid frequency of smin (the lower one
 * at a tie). Without a phase crossing gm = +Inf and wpc, Re, Im = NaN; without a gain crossing pm = +Inf and wgc, Re, Im = NaN.
 * counts [2 x N]: the kept phase crossings, the kept gain crossings. all (may be NULL) [6 x FB_MARGINS_KMAX x N]: rows w*, Re L*, Im L* of
 * the phase crossings, then of the gain crossings, slot s of row q of system i at all[(q FB_MARGINS_KMAX + s) N + i], NaN past the count.
 * Every array has the system index fastest: element (k, i) at [k N + i].
 * status [N]: 0; FB_MARGINS_NOT_FINITE: a non-finite entry of A, b, c, d or the gain; FB_MARGINS_SINGULAR: a zero or non-finite pivot, or a
 * non-finite L, at a grid point or a refinement point (a pole on the imaginary axis hit exactly). Such a system gets NaN in sel and all and
 * zero counts; the call still returns 0 and no other system changes in any bit. FB_MARGINS_TRUNCATED voids nothing.
 * Reads the handle's copy of the model, runs on its stream (fb_lss_freqresp's kernel on the grid, in slices of whole frequencies of at most
 * 2^25 one-wave workgroups each, one slice unless N nw passes 2^31 / P pairs, P = 8, 16 or 32 the smallest >= nx; then the margins' kernel)
 * and changes nothing on the handle. For the length of the call the grid response, 2 nw N doubles, is held on the device.
 * Refused, with nothing launched: a NULL or non-LSS handle, a handle without a model, a sampled handle ("a continuous-time verb on a sampled
 * model"), iu or iy out of range, a NULL w, sel, counts or status, nw outside [2, 1024], a grid entry that is not positive and finite, a grid
 * that does not strictly increase, N nw above 2^31 - 1.
 * Limits: a bracket around a lightly damped or undamped pole pair refines onto the pole (a margin near zero, or FB_MARGINS_SINGULAR);
 * crossings the grid does not bracket are not found; margins say nothing about closed-loop stability (fb_lss_poles of the closed loop does). */
enum { FB_MARGINS_NOT_FINITE = 1, FB_MARGINS_SINGULAR = 2, FB_MARGINS_TRUNCATED = 4,
       FB_MARGINS_KMAX = 8, FB_MARGINS_NX_MAX = 32 };
int32_t fb_lss_margins(fb_handle lss, int32_t iu, int32_t iy, const double* w, int32_t nw, const double* gain /* [N] or NULL */,
                       double* sel /* [10 x N] */, int32_t* counts /* [2 x N] */, double* all /* [6 x KMAX x N] or NULL */,
                       int32_t* status /* [N] */);

/* ---- sampled loops: frequency response, margins and poles of a batch of sampled models (ControlSystems' freqresp, margin, poles and damp on a
 * discrete system; the controllers of FP/control.jl run in f_periodic! at dt = 0.02 on gains designed in continuous time;
 * docs/design/linearize.md, "Sampled loops on the device") -----------------------------------------------------------------------------------
 * The three d verbs take a SAMPLED FB_MODEL_LSS handle (fb_lss_c2d, fb_lss_dlqr's closed, fb_lss_set_sampled) with a model and
 * 1 <= nx <= 32, read the handle's copy of the model (Phi, Gamma in A's and B's places), run on its stream and change nothing on it. A
 * continuous handle is refused ("a discrete-time verb on a continuous model"), as a NULL or non-LSS handle and a handle without a model are;
 * every refusal is decided before anything is launched. fb_lss_freqresp, fb_lss_margins and fb_lss_poles keep refusing a sampled handle.
 * fb_lss_set_sampled: marks a continuous handle that has a model as sampled with sample time Ts: the block in A's place is read as Phi, B's
 * as Gamma, xdot0's as delta (x+ = x0 + Phi (x - x0) + Gamma (u - u0) + delta), where fb_lss_c2d leaves them. The handle's dt becomes Ts;
 * state, inputs and clock are untouched. From then on it is a sampled handle under every verb, exactly like a result of fb_lss_c2d. This is
 * the way in for a model that is no zero-order hold of a continuous one: a loop with a sample of delay has a Phi with an eigenvalue at 0.
 * Refused: a NULL or non-LSS handle, a handle without a model, a handle that is already sampled, Ts not finite or <= 0.
 * fb_lss_dfreqresp: P(e^(j w Ts)) = c inv(z I - Phi) gamma + d of channel (iu, iy) on w [nw], 1 <= nw <= 1024, into re, im [nw x N] (system
 * index fastest; NaN where a pivot was zero or not finite), fb_lss_freqresp's layout. The host forms theta_k = w_k Ts, cos theta_k and
 * sin theta_k; no trigonometric function is evaluated on the device. Launched in slices of whole frequencies of at most 2^25 one-wave
 * workgroups, so N nw is bounded by memory only. Refused besides: iu or iy out of range, a NULL w, re or im, nw out of range, a grid entry
 * that is not positive and finite, theta_k > pi ("above the Nyquist frequency pi/Ts").
 * fb_lss_dmargins: fb_lss_margins (above) for L(z) = gain (c inv(z I - Phi) gamma + d) on the unit circle: its signature, row layouts,
 * bracket predicates, selection rules, status bits and FB_MARGINS_KMAX, frequencies in and out in rad/s. What differs: a bracket is a pair
 * of points of the circle and is refined by bisecting the arc, mid = (z_lo + z_hi) / |z_lo + z_hi|, (each component held between the ends' where it is
 * monotone along the arc), until mid equals an end in both components or after 63 halvings; the crossing is z* = the final z_lo with L* = L(z*), and w* = atan2(Im z*, Re z*) / Ts is computed by the
 * host side of this call, beside gm, pm and smin. Stage 1 is fb_lss_dfreqresp's kernel on the grid (the same bits), in its slices.
 * Refused besides: what fb_lss_dfreqresp refuses, nw outside [2, 1024], a NULL sel, counts or status, a grid whose theta does not strictly
 * increase, N nw above 2^31 - 1. Limit: a phase crossing at the Nyquist frequency itself is not bracketed (L is real there: Im L does not
 * change sign inside the grid); the limits of fb_lss_margins hold as well.
 * fb_lss_dpoles: the eigenvalues of Phi of every system, with fb_lss_poles' outputs, order (ascending |z|) and status bits (its kernel). The
 * z-plane reading (s = log(z) / Ts, natural frequency, damping) is host arithmetic (flightbatch/dfreq.py). */
int32_t fb_lss_set_sampled(fb_handle lss, double Ts);
int32_t fb_lss_dfreqresp(fb_handle lss, int32_t iu, int32_t iy, const double* w, int32_t nw, double* re, double* im);
int32_t fb_lss_dmargins(fb_handle lss, int32_t iu, int32_t iy, const double* w, int32_t nw, const double* gain /* [N] or NULL */,
                        double* sel /* [10 x N] */, int32_t* counts /* [2 x N] */, double* all /* [6 x KMAX x N] or NULL */,
                        int32_t* status /* [N] */);
int32_t fb_lss_dpoles(fb_handle lss, double* re, double* im, int32_t* iters, int32_t* status);

/* ---- connect on SAMPLED Model(lss) batches, with unit delays (the `connect`, `series` and `feedback` calls of FA design/c172/c172x_design.jl
 * on the loops FP/control.jl runs in f_periodic! every dt = 0.02; docs/design/linearize.md, "Closing sampled loops on the device") ------------
 * fb_lss_connect's contract (above) for two SAMPLED FB_MODEL_LSS handles (fb_lss_c2d, fb_lss_dlqr's closed, fb_lss_set_sampled, an earlier
 * fb_lss_dconnect) with the same Ts, bit for bit, with one element more: dz [nd] names rows of z = [y_p; y_c] that are also kept one sample,
 * q_k(t) = z[dz_k](t - 1); a row may be named more than once, a longer delay is a chain of calls. In deviation coordinates (delta, x0, u0, y0
 * play no part) the extended signal vector is ze = [y_p; y_c; q] (nz + nd rows), the extended state xe = [x_p; x_c; q] (nx' = nx_p + nx_c +
 * nd rows), and with the stacked block-diagonal (A, B, C, D) of fb_lss_connect
 *     Ae = [[A, 0], [C[dz], 0]],  Be = [B; D[dz]],  Ce = [[C, 0], [0, I]],  De = [D; 0]
 *     v = F ze[jz] + G w,  outputs ze[iz]          jz and iz index the EXTENDED vector: a read or an output is a signal now or one sample late
 *     E = inv(I - F De[jz, :]), M = E F Ce[jz, :], Nw = E G
 *     Phi' = Ae + Be M,  Gamma' = Be Nw,  C' = Ce[iz, :] + De[iz, :] M,  D' = De[iz, :] Nw
 * A delayed read adds nothing to I - F De[jz, :]: an interconnection that is ill-posed as a static one is well-posed when the signal
 * arrives a sample late. F, G, their layouts, status [N] (FB_CONNECT_NOT_FINITE, FB_CONNECT_ILL_POSED; such a system gets NaN matrices, the
 * call returns 0, no other system changes in any bit) are fb_lss_connect's. iz = NULL means every row of ze (nz + nd <= 64). With nd = 0 the
 * four matrices have the bits fb_lss_connect gives on continuous handles that hold the same matrices.
 * The new handle: an ordinary sampled FB_MODEL_LSS handle with p's Ts (dt = Ts, delta = 0), at x = 0, u = 0, t = 0, on p's device with p's
 * stream rule; fb_step runs the map. p and c are only read. Refused, with nothing launched and no handle created: everything fb_lss_connect
 * refuses for handles, sizes and NULL arguments (with nx' <= 32 and nz + nd <= FB_CONNECT_NZ_MAX in the places of nx and nz), a continuous
 * plant or compensator ("a discrete-time verb on a continuous model"), a compensator whose Ts differs from the plant's in any bit, nd
 * outside 0 .. FB_DCONNECT_ND_MAX, nd > 0 with a NULL dz, an entry of dz outside [0, nz), an entry of jz or iz outside [0, nz + nd).
 * fb_lss_connect keeps refusing a sampled handle. */
enum { FB_DCONNECT_ND_MAX = 31 };
int32_t fb_lss_dconnect(fb_handle p, fb_handle c /* NULL: no compensator */, const int32_t* dz /* [nd] or NULL */, int32_t nd,
                        const int32_t* jz, int32_t nf, const double* F, int32_t f_per_system, const double* G, int32_t g_per_system, int32_t nw,
                        const int32_t* iz, int32_t ny, int32_t* status, fb_handle* out);

/* ---- discrete PID design: the metrics of optimize_PID under the sampled law on a batch of sampled models (f_periodic! of PID,
 * FP/control.jl:431-471, the law Cessna172Xv2 and Robot2D run every dt = 0.02; FA design/pidopt.jl: Metrics :36-64, cost :66-70;
 * docs/design/linearize.md, "Discrete PID design on the device") ----------------------------------------------------------------------------
 * The plant is channel (iu, iy) of each system of a SAMPLED FB_MODEL_LSS handle with a model and 1 <= nx <= FB_DPID_NX_MAX, in deviation
 * coordinates: Phi, gamma = Gamma[:, iu], c = C[iy, :], d = D[iy, iu] (delta, x0, u0, y0 play no part). pid [4 x m x N], 1 <= m <= 64:
 * (k_p, k_i, k_d, tau_f) of candidate j of system i at pid[(f m + j) N + i] (fb_pid_metrics' layout), tau_f >= 0 (0: the plain backward
 * difference); alpha = 1 / (tau_f + Ts). bounds: NULL (no bounds) or [2 x m x N], lo then hi, lo < hi, either may be infinite.
 * Unit step of the reference from rest, ticks k = 0 .. N_t, N_t = round(t_sim / Ts), 1 <= N_t <= 200000, xi_-1 = eta_-1 = 0, sat_-1 = 0:
 *   s_k = c x_k
 *   a pair without a finite bound (the algebraic loop through d is solved: the loop is P(z) C(z) with fb_lss_dfreqresp's P):
 *       Dc = k_p + Ts k_i + alpha k_d,  u_k = (Dc (1 - s_k) + xi_k-1 - alpha eta_k-1) / (1 + d Dc),  e_k = 1 - s_k - d u_k,
 *       xi_k = xi_k-1 + Ts k_i e_k
 *   a pair with a finite bound (d must be exactly 0): e_k = 1 - s_k; halted_k = e_k sat_k-1 > 0; xi_k = xi_k-1 when halted, else
 *       xi_k-1 + Ts k_i e_k; free_k = k_p e_k + xi_k + alpha (k_d e_k - eta_k-1); u_k = clamp(free_k, lo, hi);
 *       sat_k = (free_k >= hi) - (free_k <= lo)
 *   both: eta_k = alpha tau_f eta_k-1 + Ts alpha k_d e_k;  y_k = s_k + d u_k;  x_k+1 = Phi x_k + gamma u_k
 * (a backward-Euler integrator and filtered derivative, an output clamp, an integrator that halts while the output is clamped and the error
 * pushes further into the bound; the reference block's sat_ext input and reference weights are 0 and 1.)
 * metrics [5 x m x N] (may be NULL), cost [m x N], status [m x N], weights [5] or NULL: fb_pid_metrics' definitions, row order (Ms, ie, ef,
 * iu, up) and layouts on the samples y_k, u_k, t_N = N_t Ts. Ms = min(1e3, max over the grid of 1 / |1 + P(z_j) C(z_j)|), z_j = e^(j w_j Ts),
 * C(z) = k_p + k_i Ts z / (z - 1) + k_d alpha (z - 1) / (z - alpha tau_f): the LINEAR law's sensitivity. The bounds play no part in Ms.
 * counts [2 x m x N] (may be NULL): the ticks k = 0 .. N_t with sat_k != 0, then the ticks with the integrator halted.
 * The grid w [nw] follows fb_lss_dfreqresp's rules (1 <= nw <= 1024, positive, finite, w Ts <= pi as the host computes it; the host forms
 * cos and sin, no trigonometric function is evaluated on the device); P on the grid is that verb's kernel, in its slices.
 * status: 0; FB_DPID_DIVERGED: a sample y_k or u_k was not finite or beyond 1e12 (ie, ef, iu, up and cost are +Inf, Ms is the grid's);
 * FB_DPID_SINGULAR: a zero or non-finite pivot at some grid point, or 1 + d Dc zero or not finite (the metrics are NaN, cost +Inf, counts 0);
 * FB_DPID_DIRECT: a finite bound on a system with d != 0 (the metrics are NaN, cost +Inf, counts 0). The call returns 0 in all three cases
 * and no other pair changes in any bit. Reads the handle's copy of the model, runs on its stream and changes nothing on the handle.
 * Refused, with nothing launched: a NULL or non-LSS handle, a handle without a model, a continuous handle ("a discrete-time verb on a
 * continuous model"), nx > FB_DPID_NX_MAX, m outside 1 .. 64, iu or iy out of range, a grid fb_lss_dfreqresp refuses, a negative or
 * non-finite weight or weights that sum to zero, t_sim not finite or N_t outside 1 .. 200000, tau_f < 0 or not finite, lo >= hi or a NaN
 * bound, a NULL pid, cost or status. fb_pid_metrics keeps refusing a sampled handle. */
enum { FB_DPID_DIVERGED = 1, FB_DPID_SINGULAR = 2, FB_DPID_DIRECT = 4, FB_DPID_NX_MAX = 31 };
int32_t fb_lss_dpid_metrics(fb_handle lss, int32_t iu, int32_t iy, const double* w, int32_t nw, double t_sim, const double* weights,
                            const double* pid, const double* bounds /* [2 x m x N] or NULL */, int32_t m, double* metrics, double* cost,
                            int32_t* counts /* [2 x m x N] or NULL */, int32_t* status);

/* ---- discrete LQR trackers: the sampled tracker law on a batch of sampled models (f_periodic! of LQR, FP/control.jl:708-743, the law
 * Cessna172Xv2's te2te, tv2te, vh2te, ar2ar and phibeta2ar and Robot2D's tracker run every dt = 0.02; FA design/c172/c172x_design.jl designs
 * their gains in continuous time; docs/design/linearize.md, "Discrete LQR trackers on the device") --------------------------------------------
 * fb_lss_dtracker_metrics. The plant is each system of a SAMPLED FB_MODEL_LSS handle with a model, in deviation coordinates: Phi, Gamma,
 * C_z = C[iz, :], D_z = D[iz, :] (delta, x0, u0, y0 play no part). iz [nz] names output rows; 1 <= nu <= 8, 1 <= nz <= 8,
 * nx + nu + nz <= FB_DTRACK_ROWS_MAX. A pair (system i, candidate j), 1 <= m <= 64 candidates per system, has K_fbk [nu x nx], K_fwd [nu x nz]
 * and K_int [nu x nz], host arrays with element (r, c) of pair (i, j) at [((r + rows c) m + j) N + i]. bounds: NULL (no bounds) or
 * [2 x nu x m x N], lo then hi, input r of pair (i, j) at [((s nu + r) m + j) N + i], lo < hi, either may be infinite; they bound the
 * deviation. zref [nz]: the reference step, a host array, one for the batch, finite.
 * From rest, ticks k = 0 .. N_t, N_t = round(t_sim / Ts), 1 <= N_t <= 200000, x_0 = 0, iota_-1 = 0, sat_-1 = 0, u_-1 = 0:
 *     z_k = C_z x_k + D_z u_k-1        (the law samples its command variables before it writes its output: a fed-through command is last tick's)
 *     e_k = zref - z_k;  v_k = K_int e_k;  halted_kj = v_kj sat_k-1,j > 0
 *     iota_kj = iota_k-1,j when halted, else iota_k-1,j + Ts v_kj
 *     free_k = iota_k + K_fwd zref - K_fbk x_k;  sat_k = (free_k >= hi) - (free_k <= lo);  u_k = clamp(free_k, lo, hi)
 *     x_k+1 = Phi x_k + Gamma u_k
 * (a rectangular integrator that includes the current sample, an output clamp per input, an integrator that halts, per input, while its
 * output is clamped and its input pushes further into the bound; the reference block's sat_ext is 0.) Bounds of -Inf and +Inf give the
 * bits of no bounds.
 * Outputs, each may be NULL except status. zmet [3 x nz x m x N], per command variable c at [((k nz + c) m + j) N + i]: ie, the trapezoid
 * mean of |e_c,k| over k = 0 .. N_t (fb_lss_dpid_metrics' rule); ef = |e_c,N_t|; zp = max_k |z_c,k|. umet [2 x nu x m x N], per input: iu, the
 * trapezoid mean of |u_j,k|; up = max_k |u_j,k|. counts [2 x nu x m x N], per input: the ticks with sat != 0, then the ticks with the
 * integrator halted. zs [ns x nz x m x N] and us [ns x nu x m x N]: every stride-th sample and the last one, ns =
 * fb_lss_stepinfo_samples(N_t, stride), sample s stride at row s, sample N_t at row ns - 1. status [m x N]: 0; FB_DTRACK_DIVERGED: a sample
 * of z or u was not finite or beyond 1e12 (the metrics are +Inf, the counts 0); FB_DTRACK_NOT_FINITE: a non-finite entry of Phi, Gamma, C_z,
 * D_z or of the pair's gains (the metrics are NaN, the counts 0). The samples of a flagged pair are what the arithmetic gave. The call
 * returns 0 in both cases and no other pair changes in any bit. Reads the handle's copy of the model, runs on its stream and changes
 * nothing on the handle. Refused, with nothing launched: a NULL or non-LSS handle, a handle without a model, a continuous handle ("a
 * discrete-time verb on a continuous model"), the size limits above, an entry of iz outside [0, ny), m outside 1 .. 64, t_sim not finite
 * or N_t outside 1 .. 200000, stride < 1, lo >= hi or a NaN bound, a non-finite zref, a NULL iz, gain array, zref or status.
 * fb_lss_dsteady: fb_lss_steady's contract (above) for a SAMPLED handle, with the discrete equilibrium: L_d = [Phi - I, Gamma; C_z, D_z],
 *     L_d [X; U] = [0; I],  K_fbk = K - Ts K_xi C_z  (K_xi given; else K_fbk = K),  K_fwd = U + K_fbk X
 * by the same elimination and pivot rule (the identity is subtracted while the rows are staged). K_xi [nu x nz] (may be NULL): a host array
 * under K's batch or per-system rule; with it K is the state block and K_xi the integrator block of a gain designed on the augmentation
 * [x_k; xi_k-1], xi_k = xi_k-1 + Ts z_k, and K_fbk, K_int = K_xi are the gains of the law above, whose integrator holds the current sample.
 * K_fbk [nu x nx] comes home in fb_linearize's layout and may be NULL; K_xi and K_fbk need K. status: FB_SURGERY_SINGULAR and
 * FB_SURGERY_NOT_FINITE as for fb_lss_steady (NOT_FINITE: an entry of L_d, K or K_xi); FB_DSTEADY_DIRECT: K_xi is given and D_z of that
 * system has a non-zero entry (K_fbk and K_fwd are NaN; X and U are still delivered). Refused: what fb_lss_steady refuses, and a continuous
 * handle ("a discrete-time verb on a continuous model"). fb_lss_steady keeps refusing a sampled one. */
enum { FB_DTRACK_DIVERGED = 1, FB_DTRACK_NOT_FINITE = 2, FB_DTRACK_ROWS_MAX = 32, FB_DSTEADY_DIRECT = 4 };
int32_t fb_lss_dtracker_metrics(fb_handle lss, const int32_t* iz, int32_t nz, const double* K_fbk, const double* K_fwd, const double* K_int,
                                const double* bounds /* [2 x nu x m x N] or NULL */, int32_t m, const double* zref /* [nz] */, double t_sim,
                                int32_t stride, double* zmet, double* umet, int32_t* counts, double* zs, double* us, int32_t* status);
int32_t fb_lss_dsteady(fb_handle lss, const int32_t* iz, int32_t nz, const double* K, const double* K_xi /* or NULL */, int32_t k_per_system,
                       double* X, double* U, double* K_fbk, double* K_fwd, double* rpiv, int32_t* status);

/* f_ode!(world) : FP/world.jl:26-32. Uses current x, u, s; writes xdot [N x FB_NX] (may be NULL)
 * and refreshes the output record y. */
int32_t fb_f_ode(fb_handle h, double* xdot);
/* f_step!(world) : FP/world.jl:34-39. Acts on y of the last fb_f_ode, like the reference. */
int32_t fb_f_step(fb_handle h);
/* f_periodic!(Unconditional(), world) : FP/world.jl:41-47 (no-op for C172Sv0: @no_periodic everywhere). */
int32_t fb_f_periodic(fb_handle h);
/* Cessna172Xv2: avionics.ctl.u (inputs cu [N x FB_NCU]) and the control laws' record (cs [N x FB_NCS]: s and the parts of
 * y other code reads). fb_f_periodic runs the control laws once (f_periodic!(Unconditional(), world)); fb_step runs them
 * every periodic_n steps, after the step's f_step!, on the outputs of the step's last f_ode! (FC/sim.jl:204-218). */
int32_t fb_set_ctl_inputs(fb_handle h, const double* cu);
int32_t fb_get_ctl_inputs(fb_handle h, double* cu);
int32_t fb_set_ctl_state(fb_handle h, const double* cs);
int32_t fb_get_ctl_state(fb_handle h, double* cs);
/* mdl.y of the last fb_f_ode / fb_step : y [N x FB_NY] */
int32_t fb_get_outputs(fb_handle h, double* y);
/* The same with SURVEY.md §8(b)'s field mask: only the blocks of the output record named by `field_mask` (FB_YF_* bits) cross
 * PCIe, packed one after the other in FB_Y_* order: y [N x (sum of the selected blocks' widths)] (reading `mdl.y.vehicle.kinematics`
 * alone costs 320 B per aircraft instead of 1392). fb_get_outputs(h, y) == fb_get_output_fields(h, FB_YF_ALL, y). */
enum { FB_YF_KIN = 1, FB_YF_AIR = 2, FB_YF_AERO = 4, FB_YF_LDG = 8, FB_YF_PWP = 16, FB_YF_FUEL = 32, FB_YF_DYN = 64, FB_YF_ALL = 127 };
int32_t fb_get_output_fields(fb_handle h, uint32_t field_mask, double* y);

/* nsteps x step!(sim) : FC/sim.jl:386 — RK4 (OrdinaryDiffEq, fixed dt) + callbacks in the order
 * cb_step, cb_periodic, cb_user(no-op), FC/sim.jl:204-218. Asynchronous on the handle's stream. */
int32_t fb_step(fb_handle h, int64_t nsteps);
/* steps fused per kernel launch (state stays in registers between them). Default 1. */
int32_t fb_set_steps_per_launch(fb_handle h, int32_t k);
int32_t fb_sync(fb_handle h);
/* sim.t : FC/sim.jl:261-275 */
double fb_time(fb_handle h);

/* On-device TimeSeries log: the SavingCallback of Simulation (FC/sim.jl:210-212: log = SavedValues(Float64, Y),
 * cb_save_function = deepcopy(mdl.y), :345-347) and TimeSeries(sim) (:644-704).
 * A sample = `nrows` rows for all N aircraft, taken every `every` steps after the step's callbacks (cb_save is the last
 * callback of the set, :217) into a device buffer of `capacity` samples; rows[j] in [0, Ny) selects output row y[rows[j]]
 * (an f_ode! at the saved instant refreshes y first), FB_LOG_X0 + k selects state row x[k]. every = 0 turns logging off.
 * fb_log_clear drops the samples and restarts the save phase (init!, :395-397); fb_log_record saves the current instant
 * (init! saves y(t0) through reinit!, :405-410). fb_log_read copies samples [first, first+count) to the host:
 * t [count], data [count x nrows x N] (sample slowest, aircraft fastest). fb_step fails when a sample is due and the
 * buffer is full. */
enum { FB_LOG_X0 = 1000 };
int32_t fb_log_configure(fb_handle h, int64_t every, int64_t capacity, const int32_t* rows, int32_t nrows);
int32_t fb_log_clear(fb_handle h);
int32_t fb_log_record(fb_handle h);
int32_t fb_log_count(fb_handle h, int64_t* count);
int32_t fb_log_read(fb_handle h, int64_t first, int64_t count, double* t, double* data);

/* SimulationTermination / ArgumentError mapping: per-aircraft sticky status bits (FB_ST_*). */
int32_t fb_status(fb_handle h, int32_t* status);
/* The termination record of every aircraft: step [N] = number of RK updates completed since the last init when the exception was
 * thrown (-1: not terminated), where [N] = FB_TERM_* (see above). Either pointer may be NULL. ≙ sim.t and the stack frame of the
 * exception the reference reports (FC/sim.jl:561-570). */
int32_t fb_get_termination(fb_handle h, int64_t* step, int32_t* where);
/* Checkpoint restore of that record (beside fb_set_status; there is no reference counterpart: a Julia session keeps its exception).
 * step [N], where [N] as fb_get_termination returned them; entries of aircraft whose status word is zero are ignored. Every call that
 * clears the status words (fb_trim, fb_set_state, Robot2D's fb_f_init) clears the record too; fb_set_status alone gives an
 * aircraft whose word becomes non-zero without a record (FB_TERM_OUTSIDE_STEP, the current step count). */
int32_t fb_set_termination(fb_handle h, const int64_t* step, const int32_t* where);

/* Trajectory collection across GPUs: one RCCL all-gather of the state panels over xGMI; no other
 * communication exists on this path. One process per GPU; rank 0 calls fb_comm_unique_id and the host distributes the 128
 * bytes out of band; every rank calls fb_comm_init (collective: it also exchanges the ranks' shard sizes, readable through
 * fb_comm_shard_sizes), then fb_gather_state enqueues, on the handle's stream, an all-gather of its x (DEVICE layout,
 * [N x FB_NX] or [N x FB_X2_NX] doubles, see fb_attach_state) into recv_dev (device memory, rank-major)
 * [world x Nx x n_max], n_max = the largest shard. Equal shards (n_of[r] == N on every rank): exactly [world x Nx x N], gathered
 * in place from x. Ragged shards: every rank's rows are padded to n_max through a staging copy; rank r's row k holds
 * n_of[r] valid entries at recv_dev[(r * Nx + k) * n_max ...], the rest of the row is unspecified. The handle passed to
 * fb_gather_state must be the one the communicator was initialised with (same N), otherwise the call fails. RCCL is loaded on
 * first use. */
int32_t fb_comm_unique_id(char* id128);
int32_t fb_comm_init(fb_handle h, int32_t world, int32_t rank, const char* id128, void** comm);
int32_t fb_comm_shard_sizes(void* comm, int64_t* n_of /* [world] or NULL */, int64_t* n_max /* or NULL */);
int32_t fb_gather_state(fb_handle h, void* comm, double* recv_dev);
int32_t fb_comm_destroy(void* comm);

/* Checkpoint / restore: together with fb_get/set_state, fb_get/set_inputs and (Xv2) fb_get/set_ctl_inputs|state these
 * capture everything a resumed run needs: the number of steps taken since the last init (the phase of the periodic
 * update, FC/modeling.jl:99 `_n`), sim.t, and the sticky status words (fb_set_state clears them, like init!). */
int32_t fb_get_step_count(fb_handle h, int64_t* count);
int32_t fb_set_step_count(fb_handle h, int64_t count, double t);
int32_t fb_set_status(fb_handle h, const int32_t* status);

/* ---- Scripted scenarios: `user_callback!` on the device (Cessna172Xv2, Cessna172Sv0 in fp64) ----------------------------------------
 * The reference's scenarios are closures that run after every step, behind f_step! / f_periodic! and ahead of the save (FC/sim.jl:185,
 * 204-218, 334-336): a phase symbol and, per phase, "set these inputs; if <condition on the model's outputs> set those and go on to the next
 * phase" (FA demos/c172_demos.jl:423-486 crosswind landing, :525-642 traffic pattern). For a batch the same logic is a TABLE, interpreted per
 * aircraft by a kernel that fb_step launches behind every `every`-th step (fb_step cuts its stepping launches there, as it does at the log's
 * save instants); per aircraft: a phase word (starts at 0), the step count at which the phase was entered, n_par parameter rows (host-set)
 * and n_rec record rows (written by actions, read back by the host). Nothing crosses to the host during a run.
 * One evaluation of one aircraft (status word 0 only): the `always` actions of its phase, in order; then its rules, in order — the FIRST whose
 * condition holds runs its actions and sets the next phase (at most one transition per evaluation, like the demos' if / elseif chains).
 * Blob (fb_set_table(h, FB_TABLE_SCENARIO, blob, &len, 1); doubles; integers as doubles):
 *   header [FB_SCN_HDR]:        magic 5000001, n_phase, n_rule, n_act, n_par, n_rec, 0, 0
 *   phases [n_phase][FB_SCN_PHASE_REC]: first `always` action, their number, first rule, number of rules
 *   rules  [n_rule][FB_SCN_RULE_REC]:   source kind, source row, comparison (FB_SCN_LT ...), constant c, parameter row p or -1, first action,
 *                                       number of actions, next phase.   Holds when  source - (p >= 0 ? par[p] : 0)  <cmp>  c
 *   actions [n_act][FB_SCN_ACT_REC]:    destination kind, destination row (FB_SCN_DST_UI: the bit mask), wrap flag, c0, number of terms (<= 3),
 *                                       3 x (source kind, source row, coefficient).   value = c0 + sum coefficient * source, summed in order,
 *                                       then Attitude.wrap_to_pi (FP/attitude.jl:478) if the flag is set; FB_SCN_DST_UI sets the bits where value != 0
 *                                       and clears them otherwise. A value is read when its action runs (it sees the actions before it).
 * Sources: FB_SCN_SRC_T = sim.t behind the step (steps taken x dt), T_IN_PHASE = (steps taken - step of entry) x dt, X / CS / CU / U / S = rows of
 * the state (device row order) / control-law record / control-law inputs / vehicle inputs / discrete states, PAR / REC = the aircraft's own rows,
 * and of vehicle.y at the current state: ON_GND (is_on_gnd, 0 / 1; c172.jl:998-1001), H_E, PSI / THETA / PHI (e_nb), CHI, EAS, CLM (climb rate).
 * Models: user_callback! is model-agnostic in the reference (FC/sim.jl:279), and so is the table, with what a model lacks refused when it is
 * loaded. A Cessna172Xv2 handle takes every source and destination, FB_SCN_SRC_X rows < FB_X2_NX. A Cessna172Sv0 handle created with FB_F64
 * (any mechanisation, with or without fb_set_env rows) has no control-law rows: FB_SCN_SRC_CS, FB_SCN_SRC_CU and FB_SCN_DST_CU are refused,
 * FB_SCN_SRC_X rows < FB_NX; its scripts write the vehicle's inputs (FB_SCN_DST_U, _UI: `act.u.elevator += 0.1`, c172_demos.jl:108-206) and
 * records. FB_F32 handles and Robot2D refuse the table.
 * The world as well as the aircraft (the reference's scripts set `world.atmosphere.wind.u.N / .E`, c172_demos.jl:225-228, 427-433, and may read
 * anything in mdl.y, FC/sim.jl:185, 279, 334-336), on a handle whose per-aircraft environment rows are set (fb_set_env):
 *   FB_SCN_SRC_ENV  row = FB_ENV_* (all six): the aircraft's own environment row, as fb_get_env returns it.
 *   FB_SCN_DST_ENV  row = FB_ENV_WIND_N / _E / _D only: the aircraft's wind. Written only when the value differs, and then like a changed input (the
 *                   derivative a Cessna172Xv2 handle carries between launches is dropped for that aircraft). FB_ENV_T_SL / FB_ENV_P_SL are refused: each
 *                   carries two derived rows that fb_set_env fills with the host's log / exp / sqrt, which a device write could not reproduce bit for
 *                   bit. FB_ENV_H_TERRAIN is refused: a constructor argument of HorizontalTerrain (FP/terrain.jl:34-38), not an input.
 *   FB_SCN_SRC_Y    row in [0, Ny) of fb_dims: that row of mdl.y at the state behind the step (what fb_f_ode + fb_get_outputs give at that instant),
 *                   read before any action of the evaluation runs. A table that names it makes fb_step refresh the whole output record ahead of
 *                   every evaluation (one f_ode! pass, counted by fb_timing_end among the launches); a table that does not pays nothing.
 *                   The record is the one BEFORE the evaluation's actions: after an `always` action has written the wind, FB_SCN_SRC_EAS (tapped from
 *                   the evaluation of f_ode! the walk itself makes, behind that write) and the record's EAS row differ within one evaluation.
 *                   The refresh is an fb_f_ode like any other: an aircraft whose state behind the step makes f_ode! throw gets its status bit and the
 *                   record (FB_TERM_OUTSIDE_STEP, the step count) THERE, and this very evaluation skips it. Without the kind the table would still
 *                   evaluate that aircraft, and the next stepping launch would terminate it with its own FB_TERM_* code. (The device log's save has
 *                   the same effect; here it changes what a table does.)
 * A table with either ENV kind is refused on a handle without rows (call fb_set_env first), and while it is loaded fb_set_env(h, NULL) is refused
 * (fb_scenario_configure(h, 0) first). */
enum { FB_SCN_HDR = 8, FB_SCN_PHASE_REC = 4, FB_SCN_RULE_REC = 8, FB_SCN_ACT_REC = 14, FB_SCN_NTERM = 3 };
enum { FB_SCN_SRC_CONST = 0, FB_SCN_SRC_T, FB_SCN_SRC_T_IN_PHASE, FB_SCN_SRC_X, FB_SCN_SRC_CS, FB_SCN_SRC_CU, FB_SCN_SRC_U, FB_SCN_SRC_S,
       FB_SCN_SRC_ON_GND, FB_SCN_SRC_H_E, FB_SCN_SRC_PSI, FB_SCN_SRC_THETA, FB_SCN_SRC_PHI, FB_SCN_SRC_CHI, FB_SCN_SRC_EAS, FB_SCN_SRC_CLM,
       FB_SCN_SRC_PAR, FB_SCN_SRC_REC, FB_SCN_SRC_ENV, FB_SCN_SRC_Y, FB_SCN_NSRC };
enum { FB_SCN_DST_CU = 0, FB_SCN_DST_U, FB_SCN_DST_UI, FB_SCN_DST_REC, FB_SCN_DST_ENV, FB_SCN_NDST };
enum { FB_SCN_LT = 0, FB_SCN_GT, FB_SCN_GE, FB_SCN_LE, FB_SCN_EQ, FB_SCN_NE, FB_SCN_ALWAYS };
/* fb_set_table(FB_TABLE_SCENARIO) validates every index of the blob, allocates the per-aircraft rows (phase 0, entry step 0, parameters and
 * records zero) and switches the evaluation on with every = 1. fb_scenario_configure: the period in steps (>= 1), or 0: scenario off, rows freed.
 * The scenario's state is NOT touched by fb_trim / fb_set_state (the reference's closures keep their phase across init!): set it explicitly. */
int32_t fb_scenario_configure(fb_handle h, int32_t every);
int32_t fb_scenario_set_params(fb_handle h, const double* par /* [n_par x N] */);
int32_t fb_scenario_get_params(fb_handle h, double* par /* [n_par x N] */);
int32_t fb_scenario_get_state(fb_handle h, int32_t* phase /* [N] or NULL */, int64_t* since_step /* [N] or NULL */, double* rec /* [n_rec x N] or NULL */);
int32_t fb_scenario_set_state(fb_handle h, const int32_t* phase, const int64_t* since_step, const double* rec /* each [..N] or NULL: left as is */);

/* HIP-event timing on the handle's stream around the fb_step launches issued between begin and end;
 * reports total elapsed ms and the number of stepping-kernel launches (plus the output-record refreshes of a FB_SCN_SRC_Y table). */
int32_t fb_timing_begin(fb_handle h);
int32_t fb_timing_end(fb_handle h, float* ms, int64_t* n_launches);
/* (Under a table that names FB_SCN_SRC_Y, n_launches of fb_timing_end includes the output-record refreshes, one per evaluation; the per-launch
 * stamps below cover stepping launches only, so *n of fb_timing_launches is smaller than n_launches then, and ms / n_launches is not a time per stepping launch.)
 * The same window with ONE event pair per stepping launch (both passes of a launch between its pair), up to max_launches of them;
 * after fb_timing_end, fb_timing_launches returns their durations in launch order (ms[0 .. min(*n, cap))), *n = pairs recorded.
 * A measurement aid (bench.py reports median / min / max over launches and warms up until launches agree); no reference counterpart. */
int32_t fb_timing_begin_per_launch(fb_handle h, int64_t max_launches);
int32_t fb_timing_launches(fb_handle h, float* ms, int64_t cap, int64_t* n);

/* The device math primitives of the stepping kernels, one call per element: the verb behind tests/test_gpu_math_primitives.py, which holds
 * each primitive to a long double reference in ulps (docs/design/k_step_air.md, "Math primitives, measured"). No handle: one kernel on the
 * CURRENT device's null stream, complete on return. a, b, out0, out1 are host arrays of n doubles; b may be NULL for a one-argument op and
 * out1 for a one-output op. The fp32 ops (FB_MP_F32_*) convert a, b to float on the device (pass values that are floats already) and return
 * their float results widened, which is exact.
 *   op                              a, b        out0, out1
 *   FB_MP_SQRT, FB_MP_RSQRT         x           sqrt x / 1 / sqrt x            (the hand-written fp64 forms)
 *   FB_MP_DIV                       a, b        a / b                          (fp64 division as the build's flags compile it)
 *   FB_MP_RCP                       x           1 / x
 *   FB_MP_HALF_ANGLE                y, x        cos, sin of atan2(y, x) / 2
 *   FB_MP_ATAN2_TAB(_XPOS)          y, x        atan2_tab<false> / <true>
 *   FB_MP_LOG_NEAR1                 u           log u
 *   FB_MP_SINCOS_STEP               x           sin x, cos x
 *   FB_MP_ISA_FAST, FB_MP_ISA       h, T_sl     out0 [3 x n]: T, p / p_sl, log(p / p_sl); out1: the status bits (FB_ST_ISA_RANGE) as a double
 *   FB_MP_ATAN_TABLE                k           entry min(max((int)k, 0), 32) of atan2_tab's staged table atan(k / 32)
 *   FB_MP_LIB_EXP, _LOG             x           the library's exp / log as the hot path compiles them
 *   FB_MP_LIB_SINCOS                x           the library's sin x, cos x
 *   FB_MP_LIB_ATAN2                 y, x        the library's atan2
 *   FB_MP_F32_ATAN2_FAST(_XPOS)     y, x        atan2_fast<false> / <true>
 *   FB_MP_F32_EXP_STEP, _LOG_STEP   x           exp x / log x through the base-2 hardware functions
 *   FB_MP_F32_SQRT, _RSQRT          x           sqrtf, rsqrtf
 *   FB_MP_F32_DIV                   a, b        a / b in fp32
 * Refused, with nothing launched: an op outside the two ranges, n outside 1 .. FB_MP_N_MAX, a NULL a or out0, a NULL b or out1 where the op
 * needs it. */
enum { FB_MP_SQRT = 0, FB_MP_RSQRT, FB_MP_DIV, FB_MP_RCP, FB_MP_HALF_ANGLE, FB_MP_ATAN2_TAB, FB_MP_ATAN2_TAB_XPOS, FB_MP_LOG_NEAR1,
       FB_MP_SINCOS_STEP, FB_MP_ISA_FAST, FB_MP_ISA, FB_MP_ATAN_TABLE, FB_MP_LIB_EXP, FB_MP_LIB_LOG, FB_MP_LIB_SINCOS, FB_MP_LIB_ATAN2,
       FB_MP_F64_END,
       FB_MP_F32_ATAN2_FAST = 32, FB_MP_F32_ATAN2_FAST_XPOS, FB_MP_F32_EXP_STEP, FB_MP_F32_LOG_STEP, FB_MP_F32_SQRT, FB_MP_F32_RSQRT,
       FB_MP_F32_DIV, FB_MP_F32_END,
       FB_MP_N_MAX = 1 << 24 };
int32_t fb_math_probe(int32_t op, int64_t n, const double* a, const double* b, double* out0, double* out1);

const char* fb_last_error(void);
const char* fb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLIGHTBATCH_H */
