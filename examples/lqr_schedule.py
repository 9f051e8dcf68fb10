#!/usr/bin/env python3
"""A gain schedule designed on the device: the reference's te2te autopilot lookup (throttle + elevator to throttle + elevator,
lib/FlightApps/design/c172/c172x_design.jl:149-216) for Cessna172Xv2(NED).

    trim + linearize at every (EAS, h) node        fb.linearize(world, TrimParameters(...))         on the device
    the design model: (v_x, v_y, v_z, ω_eng) -> (EAS, α, β, n_eng), the reduced longitudinal states  host numpy (get_design_model!, :23-82)
    K = lqr(P, Q, R) at every node                 fb.lqr(LinearWorld(...), Q, R)                   on the device, all nodes in one call

First the reference's own 7 x 4 nodes, with the deviation of K_fbk from the shipped te2te.h5 printed; then the same on a dense grid:
`python examples/lqr_schedule.py [nE] [nH] [device]` (default 64 x 32 nodes)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains  # noqa: E402

OMEGA_RATED = 2700.0 * 2.0 * np.pi / 60.0
SWAP = {"v_x": "EAS", "v_z": "α", "v_y": "β"}                                  # the state a design-model row replaces
LON_RED = ("q", "θ", "EAS", "α", "α_filt", "n_eng", "thr_p", "ele_p")          # XLonRed, c172x_design.jl:66
U_LON = ("throttle_cmd", "elevator_cmd")
Q_DIAG = dict(q=1.0, θ=20.0, EAS=0.02)                                         # :173-188
R_DIAG = (100.0, 5.0)


def flaps_schedule(EAS):
    return np.where(EAS < 30.0, 1.0, np.where(EAS > 35.0, 0.0, 1.0 - (EAS - 30.0) / 5.0))   # c172x_ctl.jl:18-24


def te2te_models(lss):
    """A [N, 8, 8], B [N, 8, 2] of the reduced longitudinal design model at every node"""
    xl = list(lss.x_labels)
    n = lss.A.shape[0]
    T = np.broadcast_to(np.eye(len(xl)), (n, len(xl), len(xl))).copy()
    labels = list(xl)
    for old, new in SWAP.items():
        T[:, xl.index(old), :] = lss.C[:, lss.y_labels.index(new), :]
        labels[xl.index(old)] = new
    T[:, xl.index("ω_eng"), :] = 0.0
    T[:, xl.index("ω_eng"), xl.index("ω_eng")] = 1.0 / OMEGA_RATED
    labels[xl.index("ω_eng")] = "n_eng"
    Ap = T @ lss.A @ np.linalg.inv(T)
    Bp = T @ lss.B
    ix = [labels.index(k) for k in LON_RED]
    iu = [lss.u_labels.index(k) for k in U_LON]
    return Ap[:, ix][:, :, ix], Bp[:, ix][:, :, iu]


def design(EAS, h, device):
    n = EAS.size
    w = fb.Cessna172Xv2World(n, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps_schedule(EAS)), scheme="onesided2")
    w.close()
    A, B = te2te_models(lss)
    lw = fb.LinearWorld(fb.design_model(A, B, x_labels=LON_RED, u_labels=U_LON), device=device)   # C = I, D = 0: a model to design on
    t0 = time.perf_counter()
    res = fb.lqr(lw, [Q_DIAG.get(k, 0.0) for k in LON_RED], R_DIAG)
    dt = time.perf_counter() - t0
    lw.close()
    return lss, res, dt


def main():
    nE = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    nH = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    device = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    stored = ctl_gains.load_lqr(os.path.join(ctl_gains.DATA_DIR, "te2te.h5"))
    (e0, e1), (h0, h1) = stored["bounds"].T
    K_ref = stored["K_fbk"]                                             # [2, 8, 7, 4]
    E, H = np.meshgrid(np.linspace(e0, e1, K_ref.shape[2]), np.linspace(h0, h1, K_ref.shape[3]), indexing="ij")
    lss, res, dt = design(E.ravel(order="F"), H.ravel(order="F"), device)
    K = res.K.transpose(1, 2, 0).reshape(K_ref.shape, order="F")
    print(f"te2te at the reference's {E.size} nodes: trimmed {int(lss.success.sum())}, designed {int(res.success.sum())}, "
          f"{res.iters.min()} - {res.iters.max()} iterations, residual <= {res.resid.max():.1e}, fb_lqr {dt * 1e3:.2f} ms")
    print(f"  max |K_fbk - te2te.h5| / max |te2te.h5| = {np.abs(K - K_ref).max() / np.abs(K_ref).max():.2e}")
    E, H = np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij")
    lss, res, dt = design(E.ravel(order="F"), H.ravel(order="F"), device)
    ok = res.success & lss.success
    print(f"te2te on a {nE} x {nH} grid: trimmed {int(lss.success.sum())} of {E.size}, designed {int(res.success.sum())}, "
          f"{res.iters.min()} - {res.iters.max()} iterations, residual <= {np.nanmax(res.resid):.1e}, fb_lqr {dt * 1e3:.2f} ms")
    Kq = res.K[ok][:, 1, LON_RED.index("q")]
    print(f"  elevator gain on q over the grid: {Kq.min():.4f} .. {Kq.max():.4f}")


if __name__ == "__main__":
    main()
