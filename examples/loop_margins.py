#!/usr/bin/env python3
"""Gain and phase margins of a designed loop on the device: the position-loop cell of the reference's Robot2D design notebook
(lib/FlightApps/design/robot2d/robot2d_design.ipynb), from the linearisation to the margins without a model coming home.

    linearize the default Robot2D.Vehicle                         fb.linearize(Robot2DWorld, None), fb.linear_world        on the device
    the LQR velocity tracker on (ω, v, θ) with ∫(v - v_ref):      fb.subsystem_world, fb.lqr_tracker                       on the device
        Q = diag(1e-3, 1e-2, 0), Q_int = 5e-2, R = 1e-1
    P_v: m = K_fwd v_ref - K_fbk (ω, v, θ) - ξ, ξ' = K_int (v - v_ref)    fb.connect(plant, integrator_world, ...)         on the device
    marginplot(P_v[:η, :v_ref])                                   fb.margins(P_v, u="v_ref", y="η")                        on the device
    marginplot(series(C_η2v, P_v2η)), k_p_η2v = 0.6               fb.margins(P_v, u="v_ref", y="η", gain=0.6)              on the device
    nyquistplot(...; Ms_circles = [1])                            .ms: the peak of 1 / |1 + L| over the grid
    the closed position loop v_ref = k_p (η_ref - η)              fb.connect(P_v, feedback=-k_p, ...), fb.poles            on the device

Only the tracker's gains (down, then up as the interconnection's gains) and four numbers per loop cross the bus. The margins say how far
the loop gain may change; whether the closed loop is stable is what `poles` says, printed beside them. `python examples/loop_margins.py [device]`"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402

K_P_ETA = 0.6        # C_η2v of the notebook


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    w = fb.Robot2DWorld(1, device=device)
    fb.linearize(w, None, scheme="forward")
    plant = fb.linear_world(w)
    w.close()

    red = fb.subsystem_world(plant, x=["ω", "v", "θ"])
    K_fbk, K_fwd, K_int, status = fb.lqr_tracker(red, ["v"], [1e-3, 1e-2, 0.0], np.array([[1e-1]]), [5e-2], device=device)
    red.close()
    assert (status == 0).all(), status
    K_x, k_fwd, k_int = K_fbk[0, 0], float(K_fwd[0, 0, 0]), float(K_int[0, 0, 0])

    integ = fb.integrator_world(1, device=device)
    F = np.array([[-K_x[0], -K_x[1], -K_x[2], -1.0], [0.0, k_int, 0.0, 0.0]])
    vel = fb.connect(plant, integ, feedback=F, inputs=np.array([[k_fwd], [-k_int]]), reads=["ω", "v", "θ", "ξ"], input_labels=("v_ref",))
    assert vel.ok.all()
    print(f"velocity tracker: K_fbk = {np.array2string(K_x, precision=4)}, K_fwd = {k_fwd:.4f}, K_int = {k_int:.4f}")

    for k_p in (1.0, K_P_ETA):
        m = fb.margins(vel.world, u="v_ref", y="η", gain=k_p)
        pos = fb.connect(vel.world, feedback=np.array([[-k_p]]), inputs=np.array([[k_p]]), reads=["η"], input_labels=("η_ref",))
        lam = fb.poles(pos.world)
        pos.world.close()
        print(f"η <- v_ref with k_p = {k_p:g}: GM {m.gm[0]:.3f} ({m.gm_db[0]:.2f} dB) at {m.wpc[0]:.3f} rad/s, PM {m.pm[0]:.2f}° at "
              f"{m.wgc[0]:.4f} rad/s, Ms {m.ms[0]:.2f} at {m.wms[0]:.3f} rad/s; the closed position loop is "
              f"{'stable' if lam.stable[0] else 'unstable'} (max Re pole {lam.poles[0].real.max():.3f})")
    for x in (plant, integ, vel.world):
        x.close()


if __name__ == "__main__":
    main()
