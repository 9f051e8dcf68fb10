#!/usr/bin/env python3
"""The linear half of the reference's nlsim_q demo (lib/FlightApps/demos/c172_demos.jl:135, 186),
`lsim(e2q, (x, t) -> [0.1] * (t >= 1), 0:0.01:10)`, for a BATCH of Cessna172Sv0(NED()) on the device: trim and linearise each aircraft,
take the elevator -> q channel as a LinearWorld without leaving the device, and simulate it with the zero-order-hold map
(flightbatch.timeresp.lsim: c2d at the time vector's step, then the sampled world's own step and log) — exact at the samples, where
examples/elevator_step.py integrates the same model with RK4 on the host. Beside it the RK4 line: the LinearWorld stepped with the same
input at the same dt. The two are PRINTED side by side, not asserted. `python examples/lsim_elevator.py [n]`."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402


def run(n=8, seed=0, verbose=False):
    rng = np.random.default_rng(seed)
    ac = fb.BatchedWorld(n, kinematics="NED")
    lss = fb.linearize(ac, fb.TrimParameters(EAS=rng.uniform(40.0, 52.0, n), h_e=rng.uniform(500.0, 2500.0, n)))
    assert lss.success.all()
    w = fb.linear_world(ac, u=("elevator",), y=("q",))      # e2q: every state, one input, one output
    ac.close()
    t = np.arange(0, 10.005, 0.01)
    u0 = w.u                                                  # [1, n]: the trim elevator (a fresh LinearWorld sits at its linearisation point)
    u = u0[None] + (0.1 * (t >= 1))[:, None, None]            # the demo's input on top of it
    y, _ = fb.lsim(w, u, t)                                   # the lsim line: exact at the samples
    q_zoh = y[:, 0, :]
    q_rk4 = np.empty_like(q_zoh)                              # the RK4 line: the same world stepped at the same dt
    for k in range(t.size):
        w.u = u[k]
        w.f_ode()
        q_rk4[k] = w.y[0]
        if k + 1 < t.size:
            w.step(1, dt=0.01)
    w.close()
    if verbose:
        print(f"n = {n}: q [rad/s] of aircraft 0 and {n - 1}, lsim (zero-order hold, exact) / RK4 at dt = 0.01")
        for k in range(0, t.size, 100):
            print("%5.1f" % t[k] + "".join("   %+10.6f / %+10.6f" % (q_zoh[k, i], q_rk4[k, i]) for i in (0, n - 1)))
        print("largest |lsim - RK4| over the batch and the run: %.2e rad/s (max |q| %.3f)" % (np.abs(q_zoh - q_rk4).max(), np.abs(q_zoh).max()))
    return dict(t=t, q_zoh=q_zoh, q_rk4=q_rk4)


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 8, verbose=True)
