#!/usr/bin/env python3
"""A PID gain schedule designed on the device: the reference's q2e pitch-rate loop (design_lon, lib/FlightApps/design/c172/c172x_design.jl:
222-253) for Cessna172Xv2(NED) at its 28 design nodes, from trim to PID gains.

    trim + linearize at every (EAS, h) node              fb.linearize(world, TrimParameters(...))            on the device
    the reduced longitudinal design model                host numpy (get_design_model!, :23-82; examples/lqr_schedule.py)
    te2te: K_fbk = lqr(P, Q, R), K_fwd                   fb.lqr(LinearWorld(...), Q, R); K_fwd on the host   (:149-216)
    P_q2e_opt = series(1 / s, P_te2te[q, elevator_cmd_ref])   host numpy, nx = 9                             (:224-227)
    optimize_PID(P_q2e_opt; data_0, settings, weights)   fb.optimize_pid(LinearWorld(...), ...)              on the device, all nodes per launch
    check_results(results, Metrics(Ms = 1.6, ...))       fb.check_results(results, thresholds)               (:239)

The search is a bounded pattern search, not NLopt's (docs/design/linearize.md, "PID loop design on the device"); the gains it finds are
printed beside the reference's stored q2e.h5 with the cost of both: `python examples/pid_schedule.py [device]`."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains  # noqa: E402
from lqr_schedule import LON_RED, Q_DIAG, R_DIAG, U_LON, flaps_schedule, te2te_models  # noqa: E402

T_SIM = 10.0                                                                   # :229
LOWER = fb.PIDData(k_p=0.1, k_i=0.0, k_d=0.0, τ_f=0.01)                       # :230
UPPER = fb.PIDData(k_p=10.0, k_i=50.0, k_d=2.0, τ_f=0.01)                     # :231
WEIGHTS = fb.Metrics(Ms=1.0, ie=15.0, ef=2.0, iu=0.1, up=0.0)                 # :233
DATA_0 = fb.PIDData(k_p=2.0, k_i=15.0, k_d=0.4, τ_f=0.01)                     # :234
THRESHOLDS = fb.Metrics(Ms=1.6, ie=0.3, ef=0.04, iu=np.inf, up=np.inf)        # :239


def k_fwd(A, B, K):
    """K_fwd = M22 + K M12 with M = inv([A B; C D]), z = (throttle_cmd, elevator_cmd): C = 0, D = I (:161-188)"""
    n, nx, nu = B.shape
    L = np.zeros((n, nx + nu, nx + nu))
    L[:, :nx, :nx] = A; L[:, :nx, nx:] = B; L[:, nx:, nx:] = np.eye(nu)
    M = np.linalg.inv(L)
    return M[:, nx:, nx:] + K @ M[:, :nx, nx:]


def q2e_plants(A, B, K, Kf):
    """P_q2e_opt (:224-227) at every node: the te2te loop u = K_fwd r - K_fbk x closed, the channel elevator_cmd_ref -> q, an integrator ahead"""
    n, nx, _ = B.shape
    A9 = np.zeros((n, nx + 1, nx + 1))
    A9[:, :nx, :nx] = A - B @ K
    A9[:, :nx, nx] = (B @ Kf)[:, :, U_LON.index("elevator_cmd")]
    b9 = np.zeros((n, nx + 1, 1)); b9[:, nx, 0] = 1.0
    c9 = np.zeros((n, 1, nx + 1)); c9[:, 0, LON_RED.index("q")] = 1.0
    z = np.zeros
    return fb.LinearizedSS(xdot0=z((n, nx + 1)), x0=z((n, nx + 1)), u0=z((n, 1)), y0=z((n, 1)), A=A9, B=b9, C=c9, D=z((n, 1, 1)),
                           x_labels=LON_RED + ("q_int",), u_labels=("q_err",), y_labels=("q",))


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    stored = ctl_gains.load_pid(os.path.join(ctl_gains.DATA_DIR, "q2e.h5"))
    (e0, e1), (h0, h1) = stored["bounds"].T
    nE, nH = stored["k_p"].shape
    E, H = np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij")
    EAS, h = E.ravel(order="F"), H.ravel(order="F")
    ref = np.stack([stored[k].ravel(order="F") for k in ("k_p", "k_i", "k_d", "tau_f")], axis=1)

    w = fb.Cessna172Xv2World(EAS.size, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps_schedule(EAS)), scheme="onesided2")
    w.close()
    A, B = te2te_models(lss)
    lw = fb.LinearWorld(fb.design_model(A, B, x_labels=LON_RED, u_labels=U_LON), device=device)
    te2te = fb.lqr(lw, [Q_DIAG.get(k, 0.0) for k in LON_RED], R_DIAG)
    lw.close()
    print(f"{EAS.size} nodes: trimmed {int(lss.success.sum())}, te2te designed {int(te2te.success.sum())}")

    pw = fb.LinearWorld(q2e_plants(A, B, te2te.K, k_fwd(A, B, te2te.K)), device=device)
    settings = fb.Settings(t_sim=T_SIM, lower_bounds=LOWER, upper_bounds=UPPER, dt=2e-3)
    at_ref = fb.pid_metrics(pw, ref[:, None, :], u="q_err", y="q", settings=settings, weights=WEIGHTS)
    t0 = time.perf_counter()
    opt = fb.optimize_pid(pw, u="q_err", y="q", data_0=DATA_0, settings=settings, weights=WEIGHTS)
    dt = time.perf_counter() - t0
    pw.close()
    ok = fb.check_results(opt, THRESHOLDS)
    print(f"optimize_pid: {opt.iters.min()} - {opt.iters.max()} iterations, {int(opt.evals.sum())} evaluations in {dt:.2f} s; "
          f"{int(ok.sum())} of {EAS.size} nodes pass check_results")
    print(" EAS     h   | q2e.h5  k_p     k_i    k_d   cost   | found  k_p     k_i    k_d   cost   |  Ms    ∫e     ef")
    for k in range(EAS.size):
        print(f"{EAS[k]:4.0f} {h[k]:6.0f} | {ref[k, 0]:13.4f} {ref[k, 1]:7.4f} {ref[k, 2]:6.4f} {at_ref.cost[k, 0]:.5f} | "
              f"{opt.data[k, 0]:12.4f} {opt.data[k, 1]:7.4f} {opt.data[k, 2]:6.4f} {opt.cost[k]:.5f} | "
              f"{opt.metrics[k, 0]:.3f} {opt.metrics[k, 1]:.4f} {opt.metrics[k, 2]:.4f}")


if __name__ == "__main__":
    main()
