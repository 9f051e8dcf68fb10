#!/usr/bin/env python3
"""What a sample of computational delay costs the flown pitch-rate loop, node by node, with every model on the device after c2d: the q2e
loop of the reference's longitudinal design (design_lon, lib/FlightApps/design/c172/c172x_design.jl:222-263) under the sampled PID law that
Cessna172Xv2 runs every Δt = 0.02 (f_periodic! of PID, FP/control.jl:431-471), the PID's output reaching the elevator loop in the same tick
(delay 0) or one tick later (delay 1).

    the plants P_q2e_opt at the 28 design nodes, as examples/dpid_schedule.py builds them     fb.linearize, fb.lqr, host numpy
    their zero-order hold at Ts = 0.02                                                       fb.c2d(world, 0.02)                  on the device
    the stored gains as the flown law                                                        fb.dpid_world(stored, 0.02)
    series(C, P), with and without z⁻¹ between them; margin(...)                             fb.dseries(P, C, delay=) -> fb.dmargins
    feedback(P * C), the same; poles(...), stepinfo(step(...))                               fb.dunity_feedback(P, C, delay=) -> fb.dpoles, fb.stepinfo

No model comes home after c2d: gains and index lists go up, margins, pole radii and step figures come back.
`python examples/sampled_loop_chain.py [device]`"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains  # noqa: E402
from lqr_schedule import LON_RED, Q_DIAG, R_DIAG, U_LON, flaps_schedule, te2te_models  # noqa: E402
from pid_schedule import T_SIM, k_fwd, q2e_plants  # noqa: E402

TS = 0.02


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
    sampled = fb.c2d(pw, TS)
    pw.close()
    assert sampled.ok.all()
    dw = sampled.world
    cw = fb.dpid_world(ref, TS, device=device)

    rows = []
    for delay in (0, 1):
        opn = fb.dseries(dw, cw, "q_err", "q", delay=delay)
        mg = fb.dmargins(opn.world, "e", "q")
        opn.world.close()
        loop = fb.dunity_feedback(dw, cw, "q_err", "q", delay=delay)
        lam = fb.dpoles(loop.world)
        si = fb.stepinfo(loop.world, [("q_ref", "q")], T_SIM)
        nx = loop.world.nx
        loop.world.close()
        assert opn.ok.all() and loop.ok.all() and (mg.status == 0).all() and (lam.status == 0).all()
        rows.append((mg, lam, np.abs(lam.poles).max(axis=1), si, nx))
    dw.close(); cw.close()

    (m0, l0, r0, s0, n0), (m1, l1, r1, s1, n1) = rows
    print(f"{EAS.size} nodes, Ts = {TS}: the stored q2e gains under the flown law, the PID's output applied in the same tick | one tick later "
          f"({n0} | {n1} states)")
    print(" EAS     h   |   GM            PM [deg]        ω_gc [rad/s]    1 - max |z|           overshoot [%]   settling [s]")
    for k in range(EAS.size):
        print(f"{EAS[k]:4.0f} {h[k]:6.0f} | {m0.gm[k]:6.2f} | {m1.gm[k]:5.2f}  {m0.pm[k]:6.2f} | {m1.pm[k]:6.2f}  {m0.wgc[k]:6.3f} | {m1.wgc[k]:6.3f}  "
              f"{1.0 - r0[k]:.3e} | {1.0 - r1[k]:.3e}  {s0.overshoot[k, 0]:6.2f} | {s1.overshoot[k, 0]:6.2f}  {s0.settlingtime[k, 0]:5.2f} | {s1.settlingtime[k, 0]:5.2f}")
    thumb = np.degrees(m0.wgc * TS)
    print(f"stable at {int(l0.stable.sum())} | {int(l1.stable.sum())} of {EAS.size} nodes; the delay costs {np.min(m0.pm - m1.pm):.2f}° to {np.max(m0.pm - m1.pm):.2f}° of phase margin "
          f"(ω_gc Ts = {thumb.min():.2f}° to {thumb.max():.2f}°), a factor {np.min(m0.gm / m1.gm):.2f} to {np.max(m0.gm / m1.gm):.2f} of gain margin, "
          f"{np.min(s1.overshoot[:, 0] - s0.overshoot[:, 0]):.2f} to {np.max(s1.overshoot[:, 0] - s0.overshoot[:, 0]):.2f} points of overshoot")


if __name__ == "__main__":
    main()
