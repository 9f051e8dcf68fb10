#!/usr/bin/env python3
"""Generates tests/golden/duo_pin_knots.npz ON THE GPU, from the library that is built in the tree: a DEVICE-GENERATED fixture, the
companion of duo_pin_parent.npz (make_duo_pin.py, whose `run` is used here) for everything that touches HOW A TABLE INTERVAL IS FOUND.

duo_pin_parent.npz's batch flies near trim: its angle of attack, sideslip and engine speed visit a handful of table intervals. This batch
is built to visit all of them. n = 264 Cessna172Sv0 in the WA mechanisation — one full 256-aircraft workgroup plus a ragged wave pair of
eight lanes — start from trimmed states, and on top of them

  * the body velocity keeps its magnitude and is turned so that the angle of attack takes the midpoint of every interval of the 26-knot
    (C_D) and 17-knot (C_L) axes, values between the clamp (-0.1, 0.36) and the axes' ends, and values beyond both clamps; the sideslip
    takes values in both intervals of the beta axes, beyond the +-0.2 clamp and beyond the axes' own ends (+-0.349, +-1);
  * the engine speed takes the midpoint of every interval of the 13-knot axis, from windmilling below its first knot to above its last;
  * mixture over [0, 1], manual and automatic; throttle over [0.1, 1]; engines off, starting and running;
  * the height over the terrain from H_CLEAR_LO (what a lane can lose in 21 steps kept above the 10 m clearance below which the airborne
    pass hands a lane over) to 4 km.

Every list is dealt to the lanes through a seeded permutation of its own, so the axes are not correlated. 21 steps of 0.01 s at 7 per launch.
Record it with the build a change starts from; regenerate it whenever a later change MEANS to alter rounding (and say so in that change).

    python tests/golden/make_duo_knots.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_duo_pin import run, NSTEPS, SPL, DT  # noqa: E402

OUT = os.path.join(HERE, "duo_pin_knots.npz")
N = 264
GEOID_AT_TRIM = 17.2     # EGM96 at the trim location n_e = (1, 0, 0), rounded up [m]: h_o = h_e - geoid
H_CLEAR_LO = 18.0        # lowest height over the (zero) terrain: 10 m + what 0.21 s at 55 m/s, 30 deg below the horizon, can lose (5.8 m) + 2 m
W_RATED = 2700 * np.pi / 30


def _midpoints(knots):
    k = np.unique(np.asarray(knots, dtype=np.float64))
    return 0.5 * (k[1:] + k[:-1])


def sweep_lists(tables):
    """the values each axis takes (tables: flightbatch.tables)"""
    aero, piston = tables.aero_blob(), tables.piston_blob()
    AT, PT = tables.AT, tables.PT
    k26, k17 = aero[AT["CD_ALPHA_K"]:AT["CD_ALPHA_K"] + 26], aero[AT["CL_ALPHA_K"]:AT["CL_ALPHA_K"] + 17]
    k13 = piston[PT["PISTD_N_K"]:PT["PISTD_N_K"] + 13]
    alpha = np.concatenate([_midpoints(np.concatenate([k26, k17])), [-0.3, -0.16, -0.12, -0.095, -0.0885, 0.355, 0.37, 0.45]])
    beta = np.array([-1.1, -0.45, -0.36, -0.3, -0.21, -0.15, -0.05, 0.0, 0.05, 0.15, 0.21, 0.3, 0.36, 0.45, 1.1])
    n_eng = np.concatenate([[0.03, 0.08], _midpoints(k13), [1.16, 1.25]])
    return alpha, beta, n_eng


def make_inputs(fb):
    from flightbatch import tables
    n = N
    rng = np.random.default_rng(20261019)
    w = fb.BatchedWorld(n)
    fb.f_init(w, fb.TrimParameters(EAS=rng.uniform(40.0, 55.0, n), h_e=1000.0, ψ_nb=rng.uniform(-np.pi, np.pi, n)))
    assert w.trim_success.all()
    x, s, u, ui = w.x.copy(), w.s.copy(), w.u.copy(), w.ui.copy()
    w.close()
    return shape_inputs(fb.K, tables, x, s, u, ui, rng)


def shape_inputs(K, tables, x, s, u, ui, rng):
    """the sweep on top of trimmed states (also called with the oracle's trim, to choose the sweep without a device)"""
    n = x.shape[1]
    k = np.arange(n)
    deal = lambda values: np.asarray(values)[rng.permutation(n) % len(values)]
    alpha_l, beta_l, n_eng_l = sweep_lists(tables)
    al, be = deal(alpha_l), deal(beta_l)
    v = x[K["FB_X_V_EB_B"]:K["FB_X_V_EB_B"] + 3]
    V = np.sqrt((v * v).sum(0))
    x[K["FB_X_V_EB_B"]:K["FB_X_V_EB_B"] + 3] = V * np.stack([np.cos(be) * np.cos(al), np.sin(be), np.cos(be) * np.sin(al)])   # no wind: v_wb_b = v_eb_b
    x[K["FB_X_ENG_OMEGA"]] = deal(n_eng_l) * W_RATED
    x[K["FB_X_H_E"]] = GEOID_AT_TRIM + deal(np.geomspace(H_CLEAR_LO, 4000.0, n))
    x[K["FB_X_OMEGA_EB_B"]:K["FB_X_OMEGA_EB_B"] + 3] += rng.normal(0, 0.02, (3, n))
    u[K["FB_U_THROTTLE"]] = deal(np.linspace(0.1, 1.0, n))
    u[K["FB_U_MIXTURE"]] = deal(np.linspace(0.0, 1.0, n))
    s[K["FB_S_ENG_STATE"]] = np.where(k % 5 == 1, 0, np.where(k % 5 == 4, 1, 2))       # off (windmilling) / starting / running
    ui[k % 3 == 0] &= ~np.int32(K["FB_UI_MIXTURE_AUTO"])           # manual mixture
    ui[k % 3 != 0] |= np.int32(K["FB_UI_MIXTURE_AUTO"])
    return x, s, u, ui, np.zeros(n, np.int32)


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import flightbatch as fb
    x0, s0, u, ui, st0 = make_inputs(fb)
    x, s, st = run(fb, x0, s0, u, ui, st0)
    x2, s2, st2 = run(fb, x0, s0, u, ui, st0)
    assert np.array_equal(x, x2) and np.array_equal(s, s2) and np.array_equal(st, st2), "the stepper is not deterministic run to run"
    np.savez_compressed(OUT, generated_by="device (k_step_duo<WA>), tests/golden/make_duo_knots.py",
                        x0=x0, s0=s0, u=u, ui=ui, status0=st0, dt=DT, nsteps=NSTEPS, steps_per_launch=SPL, x=x, s=s, status=st)
    print("written:", OUT, os.path.getsize(OUT), "bytes; status words:", np.unique(st).tolist())


if __name__ == "__main__":
    main()
