"""k_step_duo<WA> pinned bit for bit on a batch that visits EVERY interval of the knot axes its evaluation scans: the companion of
test_gpu_duo_constants.py for changes to how a table interval is found (grid_locate's scans, c172_device_impl.inc). That test's batch
flies near trim — a handful of intervals of the alpha, beta and engine-speed axes; this one's (tests/golden/make_duo_knots.py: 264
Cessna172Sv0, one full 256-aircraft workgroup plus a ragged wave pair of eight lanes) sweeps angle of attack, sideslip and engine speed
from beyond one end of each axis to beyond the other. tests/golden/duo_pin_knots.npz is DEVICE-GENERATED with the build before the
change that added it; x, s and status must equal it byte for byte. So that the test still means something after a regeneration, the
same run must also agree with the one-wave stepper (FLIGHTBATCH_DUO=0, which keeps the plain scan; < 1e-10 scaled as in
test_gpu_duo_constants.py) and with the oracle (< 1e-9), status words equal.

What "beyond both ends" is measured on: the values as the evaluation forms them from the state (alpha, beta from the body velocity — no
wind —, engine speed over rated speed), BEFORE the clamps of c172.jl (alpha to [-0.1, 0.36], beta to +-0.2): the clamps sit inside the
axes' ends on some sides (0.36 is the 17-knot axis' last knot, +-0.2 lies inside +-0.349), so the scans themselves see the clamped value;
the interval coverage is asserted on that clamped value.

Oracle's own run of this batch: 264 of 264 aircraft alive after the 21 steps (printed below; the condition is >= 240)."""
import os

import numpy as np
import pytest

from golden.make_duo_pin import run

pytestmark = pytest.mark.gpu

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_pin_knots.npz")
N = 264


@pytest.fixture(scope="module")
def pinned(fb):
    g = np.load(PIN)
    inputs = tuple(g[k] for k in ("x0", "s0", "u", "ui", "status0"))
    assert (int(g["nsteps"]), int(g["steps_per_launch"]), float(g["dt"])) == (21, 7, 0.01) and inputs[0].shape[1] == N
    return g, inputs, run(fb, *inputs)


@pytest.fixture(scope="module")
def oracle_run(oracle, pinned):
    _, (x0, s0, u, ui, st0), _ = pinned
    return oracle.step_term(x0, u, ui, s0, oracle.default_env(), 0.01, 21, status=st0)


def _every_interval_and_both_ends(knots, raw, seen, name):
    """`seen` (what the scan is given) falls into every interval of `knots`; `raw` (before the clamp) lies beyond both ends"""
    knots = np.asarray(knots)
    idx = np.clip(np.searchsorted(knots, seen, side="right") - 1, 0, len(knots) - 2)
    inside = (seen > knots[0]) & (seen < knots[-1])
    counts = np.bincount(idx[inside], minlength=len(knots) - 1)
    print("%-18s lanes per interval %s, below %d, above %d" % (name, counts.tolist(), int((raw < knots[0]).sum()), int((raw > knots[-1]).sum())))
    assert (counts >= 1).all(), (name, counts.tolist())
    assert (raw < knots[0]).any() and (raw > knots[-1]).any(), name


def test_batch_visits_every_interval(fb, pinned):
    from flightbatch import tables
    _, (x0, s0, u, ui, st0), _ = pinned
    K = fb.K
    AT, PT = tables.AT, tables.PT
    aero, piston = tables.aero_blob(), tables.piston_blob()
    v = x0[K["FB_X_V_EB_B"]:K["FB_X_V_EB_B"] + 3]
    assert (np.sqrt((v * v).sum(0)) > 0.1).all()                       # (airflow angles are formed above 0.1 m/s)
    alpha, beta = np.arctan2(v[2], v[0]), np.arctan2(v[1], np.sqrt(v[0] ** 2 + v[2] ** 2))
    al, be = np.clip(alpha, -0.1, 0.36), np.clip(beta, -0.2, 0.2)
    n_eng = x0[K["FB_X_ENG_OMEGA"]] / (2700 * np.pi / 30)
    assert (alpha < -0.1).any() and (alpha > 0.36).any() and (beta < -0.2).any() and (beta > 0.2).any()   # past both clamps
    _every_interval_and_both_ends(aero[AT["CD_ALPHA_K"]:AT["CD_ALPHA_K"] + 26], alpha, al, "alpha, 26 knots")
    _every_interval_and_both_ends(aero[AT["CL_ALPHA_K"]:AT["CL_ALPHA_K"] + 17], alpha, al, "alpha, 17 knots")
    _every_interval_and_both_ends(aero[AT["CY_BETA_K"]:AT["CY_BETA_K"] + 3], beta, be, "beta (C_Y)")
    _every_interval_and_both_ends(aero[AT["UNIT3_K"]:AT["UNIT3_K"] + 3], beta, be, "beta (unit axis)")
    _every_interval_and_both_ends(piston[PT["PISTD_N_K"]:PT["PISTD_N_K"] + 13], n_eng, n_eng, "engine speed")
    # the other sweeps of the batch: mixture over [0, 1] manual and automatic, throttle over [0.1, 1], every engine state, one full workgroup
    # and a ragged pair, and heights from just above the clearance below which the airborne pass hands a lane over to 4 km
    mix, thr = u[K["FB_U_MIXTURE"]], u[K["FB_U_THROTTLE"]]
    auto = (ui & K["FB_UI_MIXTURE_AUTO"]) != 0
    for sel in (auto, ~auto):
        assert mix[sel].min() < 0.02 and mix[sel].max() > 0.98
    assert thr.min() == 0.1 and thr.max() == 1.0
    assert set(np.unique(s0[K["FB_S_ENG_STATE"]]).tolist()) == {0, 1, 2} and (st0 == 0).all()
    h = x0[K["FB_X_H_E"]]
    assert x0.shape[1] == 256 + 8 and h.min() < 40.0 and h.max() > 4000.0


def test_the_airborne_pass_keeps_every_lane(fb, oracle, pinned, oracle_run):
    """the oracle's own run: nobody ends, and nobody comes within 10 m of the terrain (so k_step_duo steps every lane in every launch)"""
    import ctypes
    _, (x0, *_), _ = pinned
    xo, _, sto = oracle_run[:3]
    alive = int((sto == 0).sum())
    print("alive at the end in the oracle's run: %d of %d" % (alive, N))
    assert alive >= 240
    n_e = np.array([1.0, 0.0, 0.0])
    geoid = oracle.lib.fo_geoid_height(n_e.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    # (21 steps: the altitude is monotone between the ends for these lanes or changes by centimetres; the margin is 3 m)
    assert min(x0[fb.K["FB_X_H_E"]].min(), xo[fb.K["FB_X_H_E"]].min()) - geoid > 13.0


def test_bit_identical_to_the_recorded_parent_build(pinned):
    g, _, (x, s, st) = pinned
    dx = x != g["x"]
    print("differing state words: %d of %d (rows %s)" % (int(dx.sum()), dx.size, np.nonzero(dx.any(1))[0].tolist()))
    assert np.array_equal(st, g["status"]) and np.array_equal(s, g["s"])
    assert x.tobytes() == g["x"].tobytes()


def test_agrees_with_the_one_wave_stepper_and_the_oracle(fb, pinned, oracle_run):
    g, (x0, s0, u, ui, st0), (x, s, st) = pinned
    xa, sa, sta = run(fb, x0, s0, u, ui, st0, duo=False)
    xo, so, sto = oracle_run[:3]
    e_air = float((np.abs(x - xa) / np.maximum(np.abs(xa), 1e-3)).max())
    e_orc = float((np.abs(x - xo) / np.maximum(np.abs(xo), 1e-3)).max())
    print("max scaled difference after 21 steps: vs the one-wave stepper %.2e, vs the oracle %.2e; status words %s" % (e_air, e_orc, np.unique(st).tolist()))
    assert np.array_equal(st, sta) and np.array_equal(s, sa) and np.array_equal(st, sto) and np.array_equal(s, so)
    assert e_air < 1e-10
    assert e_orc < 1e-9
