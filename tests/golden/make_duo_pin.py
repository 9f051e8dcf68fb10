#!/usr/bin/env python3
"""Generates tests/golden/duo_pin_parent.npz ON THE GPU, from the library that is built in the tree: a DEVICE-GENERATED fixture.

It pins k_step_duo<WA>'s results bit for bit (tests/test_gpu_duo_constants.py) across changes that are meant to leave every rounding
as it is — another source for an operand, another instruction order. Record it with the build the change starts from, commit it with
the change; regenerate it whenever a later change MEANS to alter rounding (and say so in that change).

The batch: n = 200 Cessna172Sv0 in the WA mechanisation — three full wave pairs and a ragged one of eight lanes — spread over the
sphere, with, mixed into every wave: aircraft above 11 km of geopotential altitude (the stratosphere branch of the ISA model and of
the engine's temperature ratio runs beside troposphere lanes), engines off, starting and running, manual and automatic mixture, and
a few aircraft terminated before the launch. 21 steps of 0.01 s at 7 steps per launch.

    python tests/golden/make_duo_pin.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "duo_pin_parent.npz")
N, NSTEPS, SPL, DT = 200, 21, 7, 0.01


def _q_ew(lat, lon):
    """q_ew = Rz(lon) ∘ Ry(-(lat + π/2)), wander angle 0"""
    a = -(lat + np.pi / 2)
    cz, sz, cy, sy = np.cos(lon / 2), np.sin(lon / 2), np.cos(a / 2), np.sin(a / 2)
    return np.stack([cz * cy, -sz * sy, cz * sy, sz * cy])


def make_inputs(fb):
    n = N
    rng = np.random.default_rng(20261018)
    w = fb.BatchedWorld(n)
    fb.f_init(w, fb.TrimParameters(EAS=rng.uniform(40.0, 55.0, n), h_e=1000.0, ψ_nb=rng.uniform(-np.pi, np.pi, n)))
    assert w.trim_success.all()
    x, s, u, ui = w.x.copy(), w.s.copy(), w.u.copy(), w.ui.copy()
    w.close()
    K = fb.K
    k = np.arange(n)
    x[K["FB_X_Q_EW"]:K["FB_X_Q_EW"] + 4] = _q_ew(rng.uniform(-1.4, 1.4, n), rng.uniform(-np.pi, np.pi, n))
    high = k % 7 == 3                                              # above 11 km of geopotential altitude, in every wave
    x[K["FB_X_H_E"]] = np.where(high, rng.uniform(11500.0, 16000.0, n), rng.uniform(300.0, 4000.0, n))
    x[K["FB_X_OMEGA_EB_B"]:K["FB_X_OMEGA_EB_B"] + 3] += rng.normal(0, 0.02, (3, n))    # not a steady state
    u[K["FB_U_THROTTLE"]] = rng.uniform(0.1, 1.0, n)
    u[K["FB_U_MIXTURE"]] = rng.uniform(0.2, 1.0, n)
    s[K["FB_S_ENG_STATE"]] = np.where(k % 5 == 1, 0, np.where(k % 5 == 4, 1, 2))       # off (windmilling) / starting / running
    ui[k % 3 == 0] &= ~np.int32(K["FB_UI_MIXTURE_AUTO"])           # manual mixture
    st0 = np.zeros(n, np.int32)
    st0[[5, 70, 131, 195]] = K["FB_ST_NAN"]                         # terminated before the launch (one of them in the ragged pair)
    return x, s, u, ui, st0


def run(fb, x, s, u, ui, st0, duo=True):
    old = os.environ.get("FLIGHTBATCH_DUO")
    os.environ["FLIGHTBATCH_DUO"] = "1" if duo else "0"
    try:
        w = fb.BatchedWorld(x.shape[1])
    finally:
        if old is None:
            del os.environ["FLIGHTBATCH_DUO"]
        else:
            os.environ["FLIGHTBATCH_DUO"] = old
    w.set_state(x, s); w.u = u; w.ui = ui
    fb._lib.check(fb.lib.fb_set_status(w._h, st0.ctypes.data_as(C.POINTER(C.c_int32))))
    sim = fb.Simulation(w, dt=DT, save_on=False, steps_per_launch=SPL)
    fb.step(sim, NSTEPS * DT); w.sync()
    out = (w.x, w.s, w.status)
    w.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import flightbatch as fb
    x0, s0, u, ui, st0 = make_inputs(fb)
    x, s, st = run(fb, x0, s0, u, ui, st0)
    x2, s2, st2 = run(fb, x0, s0, u, ui, st0)
    assert np.array_equal(x, x2) and np.array_equal(s, s2) and np.array_equal(st, st2), "the stepper is not deterministic run to run"
    np.savez_compressed(OUT, generated_by="device (k_step_duo<WA>), tests/golden/make_duo_pin.py",
                        x0=x0, s0=s0, u=u, ui=ui, status0=st0, dt=DT, nsteps=NSTEPS, steps_per_launch=SPL, x=x, s=s, status=st)
    print("written:", OUT, os.path.getsize(OUT), "bytes; status words:", np.unique(st).tolist())


if __name__ == "__main__":
    main()
