#!/usr/bin/env python3
"""The reference's first Cessna172Sv0 demos, nlsim_q and nlsim_θ (lib/FlightApps/demos/c172_demos.jl:108-206), for a BATCH of
Cessna172Sv0(NED()): trim, fly one second from the trim condition, `act.u.elevator += a` (the demos' 0.1; here every aircraft gets its own
amplitude a_i), run to t_end — and, beside the nonlinear pitch angle θ and pitch rate q, the response of the model linearised at the same trim
(flightbatch.linearize: the demos' `linearize(world.aircraft, trim_params)` + `lsim` of the elevator channel with a step at t = 1).

Two forms of the scripted input change: `mode="callback"` — a closure after every step on the host (Simulation(..., user_callback=...): one-step
launches, the inputs over PCIe both ways) — and `mode="device"` — the same as a scenario table (flightbatch.scenario) that the device interprets
between the stepping launches; the two runs end in the same bits. The linear and the nonlinear response are PRINTED side by side, not asserted:
how far apart they are at these amplitudes is what the demo is there to show. `python examples/elevator_step.py [n] [device]`."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402

T_STEP = 1.0
ROW_THETA, ROW_Q = 13, 19   # Cessna172Sv0(NED) state rows of the C ABI: 12 vehicle rows, ψ θ φ, ϕ λ h_e, ω_eb_b, v_eb_b (include/flightbatch.h)


def scenario_table():
    """`step!(sim, 1, true); act.u.elevator += a` as phases: trim, stepped (parameter row 0: the amplitude a). The increment is read when the
    action runs — u.elevator as the trim left it, plus a — and happens once: the rule leaves the phase."""
    from flightbatch import scenario as sc
    scn = sc.Scenario(n_par=1, n_rec=0)
    TRIM, STEPPED = scn.phase("trim"), scn.phase("stepped")
    scn.when(TRIM, sc.src.T >= T_STEP, [sc.u("ELEVATOR", sc.u_("ELEVATOR") + sc.par(0))], then=STEPPED)
    return scn


def linear_response(lss, amp, t_end, dt, every):
    """lsim of the linearised aircraft with u = u0 + [0, 0, a, 0] (t >= 1): the classical RK4 on ẋ = A Δx + B Δu at the simulation's dt, sampled
    every `every` steps; returns θ [m, n] (total: y0 + Δθ, as nlsim_θ forms it) and q [m, n]."""
    n = amp.size
    iu = lss.u_labels.index("elevator")
    iq, ith = lss.y_labels.index("q"), lss.y_labels.index("θ")
    A, B = lss.A, lss.B[:, :, iu]
    f = lambda x, a: np.einsum("nij,nj->ni", A, x) + B * a[:, None]
    x = np.zeros((n, A.shape[1]))
    out_th, out_q = [], []
    nsteps = int(round(t_end / dt))
    for k in range(nsteps + 1):
        a = amp if k * dt >= T_STEP else np.zeros(n)
        if k % every == 0:
            y = lss.y0 + np.einsum("nij,nj->ni", lss.C, x) + lss.D[:, :, iu] * a[:, None]
            out_th.append(y[:, ith]); out_q.append(y[:, iq])
        k1 = f(x, a); k2 = f(x + dt / 2 * k1, a); k3 = f(x + dt / 2 * k2, a); k4 = f(x + dt * k3, a)
        x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return np.array(out_th), np.array(out_q)


def run(n=64, t_end=10.0, dt=0.02, seed=0, mode="callback", verbose=False, sample=1.0):
    K = fb.K
    rng = np.random.default_rng(seed)
    tp = fb.TrimParameters(EAS=rng.uniform(40.0, 52.0, n), h_e=rng.uniform(500.0, 2500.0, n))
    amp = rng.uniform(0.02, 0.1, n)
    w = fb.BatchedWorld(n, kinematics="NED")
    lss = fb.linearize(w, tp)      # (leaves the world trimmed in still air at the ISA sea level: the environment this run flies in)
    assert lss.success.all()
    if mode == "device":
        sim = fb.Simulation(w, dt=dt, save_on=False, steps_per_launch=50)
        w.set_scenario(scenario_table(), params=amp[None], every=1)
    else:
        done = [False]

        def callback(mdl):
            if not done[0] and mdl.t >= T_STEP:
                u = mdl.u
                u[K["FB_U_ELEVATOR"]] += amp
                mdl.u = u
                done[0] = True
        sim = fb.Simulation(w, dt=dt, save_on=False, user_callback=callback)
    fb.init(sim)
    every = int(round(sample / dt))
    theta, q = [w.x[ROW_THETA]], [w.x[ROW_Q]]
    for _ in range(int(round(t_end / sample))):
        fb.step(sim, sample); w.sync()
        x = w.x
        theta.append(x[ROW_THETA]); q.append(x[ROW_Q])
    theta, q = np.array(theta), np.array(q)
    th_lin, q_lin = linear_response(lss, amp, t_end, dt, every)
    phase = w.scenario_state()["phase"].astype(int) if mode == "device" else np.full(n, 1)
    out = dict(x=w.x, s=w.s, u=w.u, ui=w.ui, status=w.status, phase=phase, amp=amp, theta=theta, q=q, theta_lin=th_lin, q_lin=q_lin)
    if verbose:
        i_lo, i_hi = int(np.argmin(amp)), int(np.argmax(amp))
        print(f"n = {n}, mode {mode}: terminated {int((out['status'] != 0).sum())}; aircraft {i_lo} (a = {amp[i_lo]:.3f}) and {i_hi} (a = {amp[i_hi]:.3f})")
        print("   t     θ nonlinear / linear [rad]       q nonlinear / linear [rad/s]   |   θ nonlinear / linear             q nonlinear / linear")
        for k in range(theta.shape[0]):
            print("%5.1f" % (k * sample) + "".join("   %+9.5f / %+9.5f      %+9.5f / %+9.5f   " % (theta[k, i], th_lin[k, i], q[k, i], q_lin[k, i]) + ("|" if i == i_lo else "")
                                                  for i in (i_lo, i_hi)))
        print("largest |θ nonlinear - θ linear| over the batch and the run: %.4f rad; |q ...|: %.4f rad/s"
              % (np.abs(theta - th_lin).max(), np.abs(q - q_lin).max()))
    w.close()
    return out


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 64, mode="device" if "device" in sys.argv[2:] else "callback", verbose=True)
