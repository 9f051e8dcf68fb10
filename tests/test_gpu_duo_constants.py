"""k_step_duo<WA> pinned bit for bit. Role P of the wave pair keeps fp64 constants of its evaluation resident in registers it has to spare
(c172_duo_device.hpp, DuoK): the same operations on the same numbers, only the source of an operand differs — so x, s and status must equal,
byte for byte, what the build before that change gave. tests/golden/duo_pin_parent.npz is that record: DEVICE-GENERATED (tests/golden/
make_duo_pin.py, run on the GPU with the parent build), to be regenerated whenever a later change means to alter rounding.

The batch (n = 200: three full wave pairs and a ragged one of eight lanes — a resident constant is a per-lane value, valid only where it
was formed under a full EXEC mask) reaches role P's rare paths beside the common one: aircraft above 11 km of geopotential altitude in
waves that also hold troposphere lanes, engines off, starting and running, manual and automatic mixture, lanes terminated before the
launch. So that the test still means something after a regeneration, the same run must also agree with the one-wave stepper
(FLIGHTBATCH_DUO=0, < 1e-10 scaled as in test_gpu_duo.py) and with the oracle (< 1e-9)."""
import os

import numpy as np
import pytest

from golden.make_duo_pin import run

pytestmark = pytest.mark.gpu

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_pin_parent.npz")


@pytest.fixture(scope="module")
def pinned(fb):
    g = np.load(PIN)
    inputs = tuple(g[k] for k in ("x0", "s0", "u", "ui", "status0"))
    assert (int(g["nsteps"]), int(g["steps_per_launch"]), float(g["dt"])) == (21, 7, 0.01) and inputs[0].shape[1] == 200
    return g, inputs, run(fb, *inputs)


def test_batch_reaches_the_rare_paths(fb, pinned):
    g, (x0, s0, u, ui, st0), _ = pinned
    K = fb.K
    a = 6378137.0
    for wave in range(4):
        lanes = slice(64 * wave, min(64 * wave + 64, 200))
        h = x0[K["FB_X_H_E"], lanes]
        h_gp = (h - 110.0) * a / (a + h - 110.0)                      # (the geoid is within ±107 m of the ellipsoid)
        assert (h_gp > 11000.0).any() and (h < 10000.0).any()           # stratosphere and troposphere lanes in one wave
        assert set(np.unique(s0[K["FB_S_ENG_STATE"], lanes]).tolist()) == {0, 1, 2}
        assert len(np.unique(ui[lanes] & K["FB_UI_MIXTURE_AUTO"])) == 2
        assert (st0[lanes] != 0).any() and (st0[lanes] == 0).any()


def test_bit_identical_to_the_recorded_parent_build(pinned):
    g, _, (x, s, st) = pinned
    dx = x != g["x"]
    print("differing state words: %d of %d (rows %s)" % (int(dx.sum()), dx.size, np.nonzero(dx.any(1))[0].tolist()))
    assert np.array_equal(st, g["status"]) and np.array_equal(s, g["s"])
    assert np.array_equal(x, g["x"])


def test_agrees_with_the_one_wave_stepper_and_the_oracle(fb, oracle, pinned):
    g, (x0, s0, u, ui, st0), (x, s, st) = pinned
    xa, sa, sta = run(fb, x0, s0, u, ui, st0, duo=False)
    xo, so, sto, _, _ = oracle.step_term(x0, u, ui, s0, oracle.default_env(), 0.01, 21, status=st0)
    e_air = float((np.abs(x - xa) / np.maximum(np.abs(xa), 1e-3)).max())
    e_orc = float((np.abs(x - xo) / np.maximum(np.abs(xo), 1e-3)).max())
    print("max scaled difference after 21 steps: vs the one-wave stepper %.2e, vs the oracle %.2e; status words %s" % (e_air, e_orc, np.unique(st).tolist()))
    assert np.array_equal(st, sta) and np.array_equal(s, sa) and np.array_equal(st, sto) and np.array_equal(s, so)
    dead = st0 != 0
    assert np.array_equal(x[:, dead], x0[:, dead])                      # terminated before the launch: untouched
    assert (st[~dead] == 0).sum() > 150
    assert e_air < 1e-10
    assert e_orc < 1e-9
