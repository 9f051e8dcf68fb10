"""k_step_duo<WA> pinned bit for bit where a branch on the RK stage can break it. The wave-pair stepper emits a row's stage sum and stage
state in one of two forms — stages 0-2, stage 3 — chosen per emit site by a scalar branch (c172_kernels.hpp, DuoEmit<..., STAGE_EMIT>): the
same operations on the same numbers as the select it replaces, so x, s and status must equal, byte for byte, what the build before that
change gave. tests/golden/duo_stage_pin_parent.npz is that record: DEVICE-GENERATED (tests/golden/make_duo_stage_pin.py, run on the GPU with
the parent build), to be regenerated whenever a later change means to alter rounding.

What test_gpu_duo_constants.py's batch (n = 200, 21 steps, 7 per launch) does not reach: 14 steps in launches of 1, 2 and 7 — stage 3 is the
last evaluation of a launch, and a launch opens on zeroed stage sums, once per step, per two, per seven — for n = 72 (a full wave pair, a
ragged one of eight lanes and two empty ones in one workgroup) and n = 264 (a second workgroup), with lanes whose k1 is evaluated again for a
subset of their pair (f_step! modified the state), off-unit quaternions, a stall flag set within the run, engines that start, engines off
(fuel-row derivative -0.0: the sign of a zero is what a dropped or added product changes), lanes terminated before the launch and lanes
handed over in the middle of a launch. So that the test still means something after a regeneration, every run must also agree with the
one-wave stepper (FLIGHTBATCH_DUO=0, < 1e-10 scaled as in test_gpu_duo_constants.py) and with the oracle (< 1e-9)."""
import os

import numpy as np
import pytest

from golden.make_duo_stage_pin import DT, NSTEPS, PARTITIONS, SIZES, geoid, make_inputs, run

pytestmark = pytest.mark.gpu

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_stage_pin_parent.npz")


@pytest.fixture(scope="module")
def pinned():
    g = np.load(PIN)
    assert (int(g["nsteps"]), float(g["dt"]), tuple(g["partitions"].tolist())) == (NSTEPS, DT, PARTITIONS) == (14, 0.01, (1, 2, 7))
    return g


def _inputs(g, n):
    return tuple(g[f"n{n}_{k}"] for k in ("x0", "s0", "u", "ui", "status0"))


@pytest.fixture(scope="module")
def oracle_runs(oracle, pinned):
    """per batch size: the oracle's state, discrete states and status after 0 .. 14 steps (computed once, shared, left unchanged)"""
    out = {}
    for n in SIZES:
        x0, s0, u, ui, st0 = _inputs(pinned, n)
        out[n] = [oracle.step_term(x0, u, ui, s0, oracle.default_env(), DT, k, status=st0)[:3] for k in range(NSTEPS + 1)]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_batch_holds_every_kind_of_lane(fb, oracle, pinned, oracle_runs, n):
    K = fb.K
    x0, s0, u, ui, st0 = _inputs(pinned, n)
    ref = make_inputs(K, oracle, n)                                   # the recorded inputs are the generator's
    assert all(np.array_equal(a, b) for a, b in zip(ref[:5], (x0, s0, u, ui, st0)))
    assert x0.shape[1] == n and n % 64 == 8                           # full wave pairs and a ragged one of eight lanes
    hist = oracle_runs[n]
    xe, se, ste = hist[-1]
    STALL, ENG = K["FB_S_STALL"], K["FB_S_ENG_STATE"]
    live = st0 == 0
    pair = np.arange(n) // 64
    # f_step! modifies the state of SOME lanes of a pair at the first step (stall flag cleared / quaternions renormalised): k1 again for a subset
    cleared = live & (s0[STALL] == 1) & (hist[1][1][STALL] == 0)
    qn = lambda x, r: np.sqrt((x[K[r]:K[r] + 4] ** 2).sum(0))
    off_unit = live & (np.abs(qn(x0, "FB_X_Q_WB") - 1) > 1e-8) & (np.abs(qn(x0, "FB_X_Q_EW") - 1) > 1e-8)
    renormed = off_unit & (np.abs(qn(hist[1][0], "FB_X_Q_WB") - 1) < 1e-12)
    stalls = live & (s0[STALL] == 0) & (se[STALL] == 1)              # α crossed alpha_stall_hi within the run ...
    first_stall = np.array([min(k for k in range(NSTEPS + 1) if hist[k][1][STALL, i] == 1) if stalls[i] else -1 for i in range(n)])
    starts = live & (s0[ENG] == 1) & (se[ENG] == 2)                   # starting -> running, ...
    first_run = np.array([min(k for k in range(NSTEPS + 1) if hist[k][1][ENG, i] == 2) if starts[i] else -1 for i in range(n)])
    off = live & (s0[ENG] == 0) & (se[ENG] == 0)
    xd0 = oracle.f_ode(x0, u, ui, s0, oracle.default_env())[0]
    minus_zero = off & (xd0[K["FB_X_FUEL"]] == 0.0) & np.signbit(xd0[K["FB_X_FUEL"]])
    # within 10 m of the terrain (h_terrain = 0: the geoid) in the middle of a launch: above it at the start, first below it in step m (1-based)
    N = geoid(oracle, pinned[f"n{n}_lat"], pinned[f"n{n}_lon"])
    clr = np.array([h[0][K["FB_X_H_E"]] - N for h in hist])
    sinks = live & (clr[0] > 10.0) & (clr[-1] < 10.0)
    m = np.where(sinks, (clr <= 10.0).argmax(0), 0)
    mid = sinks & ((m - 1) % 7 != 0) & ((m - 1) % 2 != 0)             # the launches of 7 and of 2 steps have completed a step before it
    for p in range(n // 64 + 1):
        here = pair == p
        for name, lanes in (("stall flag cleared by the first f_step!", cleared), ("off-unit quaternions renormalised", renormed),
                            ("engine off, fuel-row derivative -0.0", minus_zero), ("handed over in the middle of a launch", mid),
                            ("engine starts", starts)):
            assert (lanes & here).any(), (name, "pair", p)
        assert 0 < (here & (cleared | renormed)).sum() < (here & live).sum()     # a subset of the pair's lanes
    assert stalls.sum() >= 2 and ((first_stall[stalls] > 1) & (first_stall[stalls] < NSTEPS)).all()    # ... not at its first or last step
    assert (first_run[starts] > 1).all() and (first_run[starts] < NSTEPS).any()
    assert (~live).any() and (~live & (pair == n // 64)).any()        # terminated before the launch, one of them in the ragged pair
    assert (ste[live] == 0).all()                                      # nobody ends within the run


@pytest.mark.parametrize("spl", PARTITIONS)
@pytest.mark.parametrize("n", SIZES)
def test_bit_identical_to_the_recorded_parent_build(fb, pinned, n, spl):
    x, s, st = run(fb, *_inputs(pinned, n), spl)
    gx, gs, gst = (pinned[f"n{n}_spl{spl}_{k}"] for k in ("x", "s", "status"))
    dx = x != gx
    print("n = %d, %d steps per launch: differing state words: %d of %d (rows %s)" % (n, spl, int(dx.sum()), dx.size, np.nonzero(dx.any(1))[0].tolist()))
    assert np.array_equal(st, gst) and np.array_equal(s, gs)
    assert np.array_equal(x.view(np.uint64), gx.view(np.uint64))      # byte for byte: the sign of a zero counts


@pytest.mark.parametrize("spl", PARTITIONS)
@pytest.mark.parametrize("n", SIZES)
def test_agrees_with_the_one_wave_stepper_and_the_oracle(fb, pinned, oracle_runs, n, spl):
    x0, s0, u, ui, st0 = _inputs(pinned, n)
    x, s, st = run(fb, x0, s0, u, ui, st0, spl)
    xa, sa, sta = run(fb, x0, s0, u, ui, st0, spl, duo=False)
    xo, so, sto = oracle_runs[n][NSTEPS]
    e_air = float((np.abs(x - xa) / np.maximum(np.abs(xa), 1e-3)).max())
    e_orc = float((np.abs(x - xo) / np.maximum(np.abs(xo), 1e-3)).max())
    print("n = %d, %d steps per launch: max scaled difference after %d steps: vs the one-wave stepper %.2e, vs the oracle %.2e; status words %s"
          % (n, spl, NSTEPS, e_air, e_orc, np.unique(st).tolist()))
    assert np.array_equal(st, sta) and np.array_equal(s, sa) and np.array_equal(st, sto) and np.array_equal(s, so)
    dead = st0 != 0
    assert np.array_equal(x[:, dead], x0[:, dead])                      # terminated before the launch: untouched
    assert e_air < 1e-10
    assert e_orc < 1e-9
