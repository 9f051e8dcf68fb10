#!/usr/bin/env python3
"""A design chain whose models stay on the device: the reference's q2e pitch-rate loop (design_lon, lib/FlightApps/design/c172/c172x_design.jl:
149-263) for Cessna172Xv2(NED) at its 28 design nodes, from trim to the closed loop's poles and step response.

    trim + linearize at every (EAS, h) node                 fb.linearize(world, TrimParameters(...))             on the device
    the reduced longitudinal design model                   host numpy (get_design_model!, :23-82; examples/lqr_schedule.py)
    te2te: K_fbk = lqr(P, Q, R)                             fb.lqr(design_world, Q, R)                           on the device   (:149-216)
    K_fwd                                                   host numpy from A, B and K_fbk                                       (:161-188)
    P_q2e_opt = series(1 / s, P_te2te[q, elevator_cmd_ref]) fb.connect(design_world, integrator_world, ...)      on the device   (:199-227)
    optimize_PID(P_q2e_opt; data_0, settings, weights)      fb.optimize_pid(q2e_world, ...)                      on the device   (:229-239)
    feedback(P_q2e_opt * C_q2e)                             fb.unity_feedback(q2e_world, pid_world(gains), ...)  on the device   (:244-263)
    dampreport, stepinfo(step(q <- q_ref))                  fb.poles, fb.stepinfo on the loop                    on the device

No model comes home between lqr and the last table: only K_fbk (down) and, with K_fwd, the gains of the interconnection (up) cross. The
design-model transform to (EAS, α, n_eng) and K_fwd stay on the host, as in the other examples: the first is surgery on the Cessna's own
rows ahead of the chain, the second needs inv([A B; C D]), which no device verb gives yet. `python examples/loop_chain.py [device]`"""
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
from pid_schedule import DATA_0, LOWER, THRESHOLDS, T_SIM, UPPER, WEIGHTS, k_fwd  # noqa: E402


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    stored = ctl_gains.load_pid(os.path.join(ctl_gains.DATA_DIR, "q2e.h5"))
    (e0, e1), (h0, h1) = stored["bounds"].T
    nE, nH = stored["k_p"].shape
    E, H = np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij")
    EAS, h = E.ravel(order="F"), H.ravel(order="F")
    n = EAS.size

    w = fb.Cessna172Xv2World(n, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps_schedule(EAS)), scheme="onesided2")
    w.close()
    A, B = te2te_models(lss)
    design = fb.LinearWorld(fb.design_model(A, B, x_labels=LON_RED, u_labels=U_LON), device=device)      # C = I: the outputs are the states

    t0 = time.perf_counter()
    te2te = fb.lqr(design, [Q_DIAG.get(k, 0.0) for k in LON_RED], R_DIAG)
    Kf = k_fwd(A, B, te2te.K)
    # u = K_fwd[:, elevator_cmd] ξ - K_fbk x; the integrator's input is the new model's input, q its output
    nx, nu = len(LON_RED), len(U_LON)
    F = np.zeros((n, nu + 1, nx + 1))
    F[:, :nu, :nx] = -te2te.K
    F[:, :nu, nx] = Kf[:, :, U_LON.index("elevator_cmd")]
    G = np.zeros((nu + 1, 1)); G[nu, 0] = 1.0
    integ = fb.integrator_world(n, device=device)
    q2e = fb.connect(design, integ, feedback=F, inputs=G, outputs=["q"], input_labels=("q_err",))

    settings = fb.Settings(t_sim=T_SIM, lower_bounds=LOWER, upper_bounds=UPPER, dt=2e-3)
    opt = fb.optimize_pid(q2e.world, u="q_err", y="q", data_0=DATA_0, settings=settings, weights=WEIGHTS)
    ok = fb.check_results(opt, THRESHOLDS)

    pid = fb.pid_world(opt.data, device=device)
    loop = fb.unity_feedback(q2e.world, pid, "q_err", "q")
    lam = fb.poles(loop.world)
    si = fb.stepinfo(loop.world, [("q_ref", "q")], T_SIM, dt=2e-3)
    dt = time.perf_counter() - t0
    for x in (design, integ, q2e.world, pid, loop.world):
        x.close()

    print(f"{n} nodes: trimmed {int(lss.success.sum())}, te2te designed {int(te2te.success.sum())}, q2e plants connected {int(q2e.ok.sum())}, "
          f"{int(ok.sum())} pass check_results, loops closed {int(loop.ok.sum())}, stable {int(lam.stable.sum())}; lqr to stepinfo {dt:.2f} s")
    print(" EAS     h   |  k_p     k_i    k_d   |  Ms    ∫e     ef   | max Re pole  ζ min | rise time  settling time  overshoot")
    for k in range(n):
        p = lam.poles[k]
        print(f"{EAS[k]:4.0f} {h[k]:6.0f} | {opt.data[k, 0]:6.3f} {opt.data[k, 1]:7.3f} {opt.data[k, 2]:6.3f} | {opt.metrics[k, 0]:.3f} "
              f"{opt.metrics[k, 1]:.4f} {opt.metrics[k, 2]:.4f} | {p.real.max():11.2e} {lam.zeta[k].min():6.3f} | {si.risetime[k, 0]:8.3f} s "
              f"{si.settlingtime[k, 0]:11.3f} s {si.overshoot[k, 0]:8.2f} %")


if __name__ == "__main__":
    main()
