#!/usr/bin/env python3
"""How far is a continuous design from the sampled optimum at the autopilot's rate? The reference designs its gains in continuous time
(lqr(P, Q, R), lib/FlightApps/design/c172/c172x_design.jl) and holds them between the samples of f_periodic! at Δt = 0.02 (FP/control.jl).
For a batch of Cessna172Sv0(NED()) at the design nodes of the te2te lookup, on the longitudinal states examples/lqr_schedule.py designs on:

    trim + linearize at every (EAS, h) node        fb.linearize(world, TrimParameters(...))               on the device
    the longitudinal subsystem                     fb.linear_world(world, x=, u=, y=)                     device to device
    K_c = lqr(P, Q, R)                             fb.lqr(w, Q, R)                                        on the device
    K_d = lqr(Discrete, Φ, Γ, Ts Q, Ts R)          fb.dlqr(fb.c2d(w, 0.02).world, 0.02 Q, 0.02 R)         on the device

Printed per node: the largest relative difference of the two gains, and the spectral radius of Φ − Γ K (host numpy) under either of them:
the sampled closed loop of the gain that is actually held. `python examples/dlqr_schedule.py [nE] [nH] [device]` (default: the 7 x 4 nodes)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains  # noqa: E402

TS = 0.02                                                                       # the autopilot's Δt
LON = dict(x=("q", "θ", "v_x", "v_z", "α_filt", "ω_eng"), u=("throttle", "elevator"), y=("q", "θ", "α", "EAS"))
Q_DIAG = dict(q=1.0, θ=20.0, v_x=0.02)                                          # c172x_design.jl:173-188, v_x in EAS's place
R_DIAG = (100.0, 5.0)


def main():
    stored = ctl_gains.load_lqr(os.path.join(ctl_gains.DATA_DIR, "te2te.h5"))
    (e0, e1), (h0, h1) = stored["bounds"].T
    nE = int(sys.argv[1]) if len(sys.argv) > 1 else stored["K_fbk"].shape[2]
    nH = int(sys.argv[2]) if len(sys.argv) > 2 else stored["K_fbk"].shape[3]
    device = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    E, H = (a.ravel(order="F") for a in np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij"))
    ac = fb.BatchedWorld(E.size, kinematics="NED", device=device)
    lss = fb.linearize(ac, fb.TrimParameters(EAS=E, h_e=H))
    w = fb.linear_world(ac, **LON)
    ac.close()
    Q, R = np.array([Q_DIAG.get(k, 0.0) for k in LON["x"]]), np.array(R_DIAG)
    cont = fb.lqr(w, Q, R)
    s = fb.c2d(w, TS)
    disc = fb.dlqr(s.world, TS * Q, TS * R)
    Phi, Gam = s.world.model()
    s.world.close()
    w.close()
    ok = lss.success & (lss.status == 0) & cont.success & s.ok & disc.success
    print(f"Cessna172Sv0(NED), {nE} x {nH} = {E.size} nodes, states {' '.join(LON['x'])}, Ts = {TS}: trimmed, linearised and designed twice at "
          f"{int(ok.sum())}; fb_lqr {cont.iters.min()} - {cont.iters.max()} iterations, fb_lss_dlqr {disc.iters.min()} - {disc.iters.max()} doublings, "
          f"residual <= {np.nanmax(disc.resid):.1e}")
    print("   EAS      h    max|K_d - K_c| / max|K_c|    rho(Phi - Gam K_c)    rho(Phi - Gam K_d)")
    rho = lambda M: float(np.abs(np.linalg.eigvals(M)).max())
    for i in np.flatnonzero(ok):
        d = np.abs(disc.K[i] - cont.K[i]).max() / np.abs(cont.K[i]).max()
        print(f"  {E[i]:5.1f}  {H[i]:6.0f}   {d:12.3e}                 {rho(Phi[i] - Gam[i] @ cont.K[i]):.6f}              {rho(Phi[i] - Gam[i] @ disc.K[i]):.6f}")


if __name__ == "__main__":
    main()
