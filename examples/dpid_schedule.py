#!/usr/bin/env python3
"""The q2e pitch-rate loop under the law as it flies: the reference's stored q2e gains were designed on the continuous compensator
(examples/pid_schedule.py; design_lon, lib/FlightApps/design/c172/c172x_design.jl:222-253), but Cessna172Xv2 runs the sampled PID
(f_periodic! of PID, FP/control.jl:431-471) every Δt = 0.02 with τ_f = 0.01, half the sample time. At the 28 design nodes:

    the plants P_q2e_opt, as examples/pid_schedule.py builds them      fb.linearize, fb.lqr, host numpy
    their zero-order hold at Ts = 0.02                                  fb.c2d(world, 0.02)                              on the device
    the stored gains: continuous metrics beside the flown law's        fb.pid_metrics | fb.dpid_metrics                 on the device
    the search under the flown law, from the stored gains              fb.optimize_dpid(world, data_0=stored, ...)      all nodes per launch
    the same with the PID's output held to [-1, 3]                     fb.optimize_dpid(..., bounds=(-1, 3))

Ms is the sensitivity peak of the linear law on the grid; the bounds play no part in it. `python examples/dpid_schedule.py [device]`."""
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
from pid_schedule import LOWER, T_SIM, THRESHOLDS, UPPER, WEIGHTS, k_fwd, q2e_plants  # noqa: E402

TS = 0.02
OUT_BOUNDS = (-1.0, 3.0)


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
    pw = fb.LinearWorld(q2e_plants(A, B, te2te.K, k_fwd(A, B, te2te.K)), device=device)
    settings = fb.Settings(t_sim=T_SIM, lower_bounds=LOWER, upper_bounds=UPPER, dt=1e-3)
    cont = fb.pid_metrics(pw, ref[:, None, :], u="q_err", y="q", settings=settings, weights=WEIGHTS)
    sampled = fb.c2d(pw, TS)
    pw.close()
    dw = sampled.world
    box = fb.Settings(t_sim=T_SIM, lower_bounds=fb.PIDData(*np.minimum(np.asarray(LOWER), ref.min(axis=0))),
                      upper_bounds=fb.PIDData(*np.maximum(np.asarray(UPPER), ref.max(axis=0))))
    flown = fb.dpid_metrics(dw, ref[:, None, :], u="q_err", y="q", settings=box, weights=WEIGHTS)
    t0 = time.perf_counter()
    opt = fb.optimize_dpid(dw, u="q_err", y="q", data_0=ref, settings=box, weights=WEIGHTS)
    dt = time.perf_counter() - t0
    held_ref = fb.dpid_metrics(dw, ref[:, None, :], u="q_err", y="q", settings=box, weights=WEIGHTS, bounds=OUT_BOUNDS)
    held = fb.optimize_dpid(dw, u="q_err", y="q", data_0=ref, settings=box, weights=WEIGHTS, bounds=OUT_BOUNDS)
    dw.close()

    ok_c, ok_f, ok_o = (fb.check_results(m, THRESHOLDS) for m in (cont.metrics[:, 0], flown.metrics[:, 0], opt.metrics))
    print(f"{EAS.size} nodes, Ts = {TS}: the stored gains pass Ms < {THRESHOLDS.Ms}, ∫e < {THRESHOLDS.ie}, ef < {THRESHOLDS.ef} at {int(ok_c.sum())} nodes on the "
          f"continuous compensator and at {int(ok_f.sum())} under the flown law; the gains found under the flown law at {int(ok_o.sum())}")
    print(f"optimize_dpid from the stored gains: {opt.iters.min()} - {opt.iters.max()} iterations, {int(opt.evals.sum())} evaluations in {dt:.2f} s")
    print(" EAS     h   | stored: Ms cont. flown   ∫e cont. flown  cost cont. flown | found   k_p     k_i    k_d   Ms    cost  | "
          f"held to [{OUT_BOUNDS[0]:g}, {OUT_BOUNDS[1]:g}]: cost stored, found, clamped ticks")
    for k in range(EAS.size):
        print(f"{EAS[k]:4.0f} {h[k]:6.0f} | {cont.metrics[k, 0, 0]:14.3f} {flown.metrics[k, 0, 0]:6.3f} {cont.metrics[k, 0, 1]:9.4f} {flown.metrics[k, 0, 1]:.4f} "
              f"{cont.cost[k, 0]:10.5f} {flown.cost[k, 0]:.5f} | {opt.data[k, 0]:11.4f} {opt.data[k, 1]:7.4f} {opt.data[k, 2]:6.4f} {opt.metrics[k, 0]:.3f} {opt.cost[k]:.5f} | "
              f"{held_ref.cost[k, 0]:.5f} {held.cost[k]:.5f} {int(held_ref.counts[k, 0, 0]):4d}")


if __name__ == "__main__":
    main()
