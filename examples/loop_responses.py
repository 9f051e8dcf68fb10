#!/usr/bin/env python3
"""Step responses of designed loops on the device: `step(P[:y, :u], t_sim) |> stepinfo` as the reference's design material uses it.

  1. The two StepInfo tables the robot2d design notebook stores (lib/FlightApps/design/robot2d/robot2d_design.ipynb), end to end:
         linearize the default Robot2D.Vehicle                 fb.linearize(Robot2DWorld, None)          on the device
         the LQR velocity loop v <- v_ref, the position loop     host numpy from the device's A, B and robot2d.h5's gains
         η <- η_ref with v_ref = 0.6 (η_ref - η)
         stepinfo(step(...))                                    fb.stepinfo(LinearWorld(...), ...)         on the device
     printed beside the stored text. The notebook's sample times are not recorded; 0.0062 s and 0.005 s are the ones every printed time is a
     multiple of (docs/design/linearize.md, "Step responses on the device").
  2. q <- q_ref of the q2e pitch-rate loop of Cessna172Xv2(NED) at the 28 design nodes with the stored PID gains (q2e.h5), the plants built
     as in examples/pid_schedule.py: rise time, settling time and overshoot per node, one launch.

`python examples/loop_responses.py [device]`"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains, hdf5_min  # noqa: E402
from lqr_schedule import LON_RED, Q_DIAG, R_DIAG, U_LON, flaps_schedule, te2te_models  # noqa: E402
from pid_schedule import T_SIM, k_fwd, q2e_plants  # noqa: E402

K_P_ETA = 0.6        # C_η2v of the notebook


def one_channel(A, b, c, u, y):
    """[n, nx, nx], [n, nx], [n, nx] -> a one-input, one-output LinearizedSS batch with D = 0"""
    n, nx = b.shape
    z = np.zeros
    return fb.LinearizedSS(xdot0=z((n, nx)), x0=z((n, nx)), u0=z((n, 1)), y0=z((n, 1)), A=A, B=b[:, :, None].copy(), C=c[:, None, :].copy(),
                           D=z((n, 1, 1)), x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=(u,), y_labels=(y,))


def robot2d_loops(A, B):
    """the velocity loop (states ω, v, θ, η, ξ: m = K_fwd v_ref - K_x (ω, v, θ) - ξ, ξ' = K_int (v - v_ref)) and the position loop around it"""
    g = hdf5_min.read_all(os.path.join(ROOT, "flight.jl_amd", "data", "robot2d.h5"))
    K_x, K_fwd, K_int = g["K_fbk"].ravel()[:3], float(g["K_fwd"].ravel()[0]), float(g["K_int"].ravel()[0])
    Kfull = np.concatenate([K_x, [0.0]])[None, :]
    Cv = np.array([[0.0, 1.0, 0.0, 0.0]])
    Av = np.block([[A - B @ Kfull, -B], [K_int * Cv, np.zeros((1, 1))]])
    bv = np.concatenate([B[:, 0] * K_fwd, [-K_int]])
    cv, ce = np.array([0.0, 1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0, 0.0])
    return (Av, bv, cv), (Av - K_P_ETA * np.outer(bv, ce), K_P_ETA * bv, ce)


def pid_loops(plants, gains):
    """r -> y of the unity-feedback loop of each plant (A, b, c; d = 0) with C(s) = k_p + k_i / s + k_d s / (tau_f s + 1): states (x, ξ, η) with
    ξ' = e, η' = (e - η) / tau_f, u = k_p e + k_i ξ + (k_d / tau_f)(e - η), e = r - c x"""
    A, b, c = plants.A, plants.B[:, :, 0], plants.C[:, 0, :]
    n, nx = b.shape
    kp, ki, kd, tf = gains.T
    Dc = kp + kd / tf
    urow = np.concatenate([-Dc[:, None] * c, ki[:, None], -(kd / tf)[:, None]], axis=1)
    yrow = np.concatenate([c, np.zeros((n, 2))], axis=1)
    M = np.zeros((n, nx + 2, nx + 2))
    M[:, :nx, :nx] = A
    M[:, :nx, :] += b[:, :, None] * urow[:, None, :]
    M[:, nx, :] = -yrow
    M[:, nx + 1, :] = -yrow / tf[:, None]
    M[:, nx + 1, nx + 1] -= 1.0 / tf
    c0 = np.concatenate([b * Dc[:, None], np.ones((n, 1)), (1.0 / tf)[:, None]], axis=1)
    return M, c0, yrow


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0

    # ---- 1. the notebook's two tables
    w = fb.Robot2DWorld(1, device=device)
    lss = fb.linearize(w, None, scheme="forward")
    w.close()
    stored = json.load(open(os.path.join(ROOT, "tests", "golden", "robot2d_stepinfo.json"), encoding="utf-8"))
    loops = dict(zip(("velocity_loop", "position_loop"), robot2d_loops(lss.A[0], lss.B[0])))
    names = {"velocity_loop": ("v_ref", "v"), "position_loop": ("η_ref", "η")}
    for which, (A, b, c) in loops.items():
        t = stored[which]
        u, y = names[which]
        lw = fb.LinearWorld(one_channel(A[None], b[None], c[None], u, y), device=device)
        si = fb.stepinfo(lw, [(u, y)], t["t_sim"], dt=t["dt"])
        stable = bool(fb.poles(lw).stable[0])
        auto = fb.timeresp.default_dt(lw)
        lw.close()
        print(f"{which.replace('_', ' ')}, {y} <- {u}, t_sim = {t['t_sim']:g}, dt = {t['dt']:g} (default_dt would be {auto:g}); stable: {stable}")
        print(f"{'on the device':<30s}{'the notebook':<30s}")
        for got, ref in zip(si.show(0, 0).split("\n"), t["lines"]):
            print(f"{got:<30s}{ref:<30s}")
        print()

    # ---- 2. q <- q_ref at the 28 design nodes with the stored gains
    gains = ctl_gains.load_pid(os.path.join(ctl_gains.DATA_DIR, "q2e.h5"))
    (e0, e1), (h0, h1) = gains["bounds"].T
    nE, nH = gains["k_p"].shape
    E, H = np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij")
    EAS, h = E.ravel(order="F"), H.ravel(order="F")
    ref = np.stack([gains[k].ravel(order="F") for k in ("k_p", "k_i", "k_d", "tau_f")], axis=1)
    w = fb.Cessna172Xv2World(EAS.size, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps_schedule(EAS)), scheme="onesided2")
    w.close()
    A, B = te2te_models(lss)
    lw = fb.LinearWorld(fb.design_model(A, B, x_labels=LON_RED, u_labels=U_LON), device=device)
    te2te = fb.lqr(lw, [Q_DIAG.get(k, 0.0) for k in LON_RED], R_DIAG)
    lw.close()
    M, c0, yrow = pid_loops(q2e_plants(A, B, te2te.K, k_fwd(A, B, te2te.K)), ref)
    cw = fb.LinearWorld(one_channel(M, c0, yrow, "q_ref", "q"), device=device)
    si = fb.stepinfo(cw, [("q_ref", "q")], T_SIM, dt=2e-3)
    stable = fb.poles(cw).stable
    cw.close()
    print(f"q <- q_ref of the q2e loop with the stored gains, t_sim = {T_SIM:g}, dt = 0.002: {int(si.ok.sum())} of {EAS.size} nodes ok, "
          f"{int(stable.sum())} stable")
    print(" EAS     h   |  k_p     k_i    k_d   | rise time  settling time  overshoot  final value")
    for k in range(EAS.size):
        print(f"{EAS[k]:4.0f} {h[k]:6.0f} | {ref[k, 0]:6.3f} {ref[k, 1]:7.3f} {ref[k, 2]:6.3f} | {si.risetime[k, 0]:8.3f} s {si.settlingtime[k, 0]:11.3f} s "
              f"{si.overshoot[k, 0]:8.2f} % {si.yf[k, 0]:10.4f}")


if __name__ == "__main__":
    main()
