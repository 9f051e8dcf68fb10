#!/usr/bin/env python3
"""The batch form of the reference's nlsim_θ demo (lib/FlightApps/demos/c172_demos.jl:108-206) with BOTH models on the device: a batch of
Cessna172Sv0(NED()) is trimmed and linearised there (flightbatch.linearize), `Model(lss)` is built from that result device to device
(flightbatch.linear_world) and stepped beside the nonlinear batch: one second at the trim condition, then `elevator += a_i`, then on to t_end.

The nonlinear batch gets its input change from a scenario table the device interprets; the linear batch gets its input row once, between two
fb_step calls. Both record θ and q once per second in their on-device logs. What crosses PCIe: the amplitudes and the linear input row up,
the two logs down at the end (and, inside flightbatch.linearize, the host copy of the LinearizedSS that the linear run does not use).
The responses are PRINTED side by side, not asserted: how far apart they are at these amplitudes is what the demo shows
(examples/elevator_step.py steps the same linear model with numpy on the host). `python examples/linear_vs_nonlinear.py [n] [device]`."""
import ctypes as C
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
from elevator_step import ROW_Q, ROW_THETA, T_STEP, scenario_table  # noqa: E402


def _log(h, n, nrows):
    cnt = C.c_int64()
    check(fb.lib.fb_log_count(h, C.byref(cnt)))
    t, data = np.zeros(cnt.value), np.zeros((cnt.value, nrows, n))
    check(fb.lib.fb_log_read(h, 0, cnt.value, t.ctypes.data_as(C.POINTER(C.c_double)), data.ctypes.data_as(C.POINTER(C.c_double))))
    return t, data


def run(n=64, t_end=10.0, dt=0.02, seed=0, device=0, sample=1.0, verbose=False):
    rng = np.random.default_rng(seed)
    tp = fb.TrimParameters(EAS=rng.uniform(40.0, 52.0, n), h_e=rng.uniform(500.0, 2500.0, n))
    amp = rng.uniform(0.02, 0.1, n)
    every, nsamp = int(round(sample / dt)), int(round(t_end / sample))
    w = fb.BatchedWorld(n, device=device, kinematics="NED")
    assert fb.linearize(w, tp).success.all()        # (leaves the world trimmed, and the LinearizedSS on the device)
    lw = fb.linear_world(w)                         # Model(lss): x = x0, u = u0, the world's dt
    # the nonlinear batch: scenario table for the step, device log of the state rows θ and q
    sim = fb.Simulation(w, dt=dt, save_on=False, steps_per_launch=every)
    w.set_scenario(scenario_table(), params=amp[None], every=1)
    rows = np.array([fb.K["FB_LOG_X0"] + ROW_THETA, fb.K["FB_LOG_X0"] + ROW_Q], dtype=np.int32)
    check(fb.lib.fb_log_configure(w._h, every, nsamp + 1, rows.ctypes.data_as(C.POINTER(C.c_int32)), 2))
    fb.init(sim)
    check(fb.lib.fb_log_record(w._h))               # the sample at t = 0
    # the linear batch: the same clock, the output rows θ and q
    lw.log_configure(every=every, capacity=nsamp + 1, y=("θ", "q"))
    check(fb.lib.fb_log_record(lw._h))
    k_step = int(round(T_STEP / dt))
    fb.step(sim, t_end)
    lw.step(k_step, dt=dt, steps_per_launch=every)
    u = lw.u
    u[lw.u_labels.index("elevator")] += amp
    lw.u = u
    lw.step(nsamp * every - k_step)
    w.sync(); lw.sync()
    t_nl, d_nl = _log(w._h, n, 2)
    t_l, d_l = lw.log_read()
    out = dict(t=t_nl, amp=amp, theta=d_nl[:, 0], q=d_nl[:, 1], theta_lin=d_l[:, 0], q_lin=d_l[:, 1], t_lin=t_l, status=w.status)
    if verbose:
        i_lo, i_hi = int(np.argmin(amp)), int(np.argmax(amp))
        print(f"n = {n}: terminated {int((out['status'] != 0).sum())}; aircraft {i_lo} (a = {amp[i_lo]:.3f}) and {i_hi} (a = {amp[i_hi]:.3f}); both models stepped on the device")
        print("   t     θ nonlinear / linear [rad]       q nonlinear / linear [rad/s]   |   θ nonlinear / linear             q nonlinear / linear")
        for k in range(len(t_nl)):
            print("%5.1f" % t_nl[k] + "".join("   %+9.5f / %+9.5f      %+9.5f / %+9.5f   " % (out["theta"][k, i], out["theta_lin"][k, i], out["q"][k, i], out["q_lin"][k, i])
                                             + ("|" if i == i_lo else "") for i in (i_lo, i_hi)))
        print("largest |θ nonlinear - θ linear| over the batch and the run: %.4f rad; |q ...|: %.4f rad/s"
              % (np.abs(out["theta"] - out["theta_lin"]).max(), np.abs(out["q"] - out["q_lin"]).max()))
    lw.close(); w.close()
    return out


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 64, device=int(sys.argv[2]) if len(sys.argv) > 2 else 0, verbose=True)
