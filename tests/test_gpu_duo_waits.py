"""k_step_duo<WA> pinned bit for bit where the pair's synchronisation can break it. The two waves of a pair keep in step through two counters
in LDS (c172_kernels.hpp, DuoSync): a wave publishes the points it has passed and polls its partner's counter where it needs something of it.
How the poll is built — scalar or per lane, how long a failed pass sleeps, who wakes whom — changes no operation of the evaluation, so x, s
and status must equal, byte for byte, what the build before such a change gave. A wrong wait shows as a stale hand-over (wrong bits) or as
FB_ST_NAN from a wait that ran into its bound. tests/golden/duo_waits_pin_parent.npz is the record: DEVICE-GENERATED (tests/golden/
make_duo_waits_pin.py, run on the GPU with the parent build), to be regenerated whenever a later change means to alter rounding.

The batch (n = 328: a full workgroup, and a second one with a full pair, a ragged pair of eight lanes and two empty pairs) makes the roles
arrive in every order: stratosphere lanes beside troposphere lanes in every pair that runs (role P late at its points A and W), engines
off, starting and running, lanes whose k1 is evaluated again for a part of their pair, a pair terminated before the launch (the "nobody
runs" publications) and a pair whose lanes all sink through 10 m of clearance in the middle of a launch (the pair leaves: EXIT word).
14 steps in launches of 1, 2 and 7. So that the test still means something after a regeneration, every run must also agree with the
one-wave stepper (FLIGHTBATCH_DUO=0, < 1e-10 scaled as in test_gpu_duo_constants.py) and with the oracle (< 1e-9)."""
import os

import numpy as np
import pytest

from golden.make_duo_waits_pin import CROSS_AT, DEAD_PAIR, DT, N, NSTEPS, PARTITIONS, SINK_PAIR, kinds, make_inputs, run
from golden.make_duo_stage_pin import geoid

pytestmark = pytest.mark.gpu

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_waits_pin_parent.npz")


@pytest.fixture(scope="module")
def pinned():
    g = np.load(PIN)
    assert (int(g["nsteps"]), float(g["dt"]), tuple(g["partitions"].tolist())) == (NSTEPS, DT, PARTITIONS) == (14, 0.01, (1, 2, 7))
    assert g["x0"].shape[1] == N == 328
    return g


def _inputs(g):
    return tuple(g[k] for k in ("x0", "s0", "u", "ui", "status0"))


@pytest.fixture(scope="module")
def oracle_runs(oracle, pinned):
    """the oracle's state, discrete states and status after 0 .. 14 steps (computed once, shared, left unchanged)"""
    x0, s0, u, ui, st0 = _inputs(pinned)
    return [oracle.step_term(x0, u, ui, s0, oracle.default_env(), DT, k, status=st0)[:3] for k in range(NSTEPS + 1)]


@pytest.fixture(scope="module")
def device_runs(fb, pinned):
    """per partition: the wave-pair stepper twice and the one-wave stepper once (computed once, shared, left unchanged)"""
    inp = _inputs(pinned)
    return {spl: (run(fb, *inp, spl), run(fb, *inp, spl), run(fb, *inp, spl, duo=False)) for spl in PARTITIONS}


def test_batch_reaches_what_it_claims(fb, oracle, pinned, oracle_runs):
    K = fb.K
    x0, s0, u, ui, st0 = _inputs(pinned)
    ref = make_inputs(K, oracle)                                      # the recorded inputs are the generator's
    assert all(np.array_equal(a, b) for a, b in zip(ref[:5], (x0, s0, u, ui, st0)))
    n = N
    kind = kinds()
    pair = np.arange(n) // 64
    assert n == 256 + 64 + 8                                          # a full workgroup; a full pair, a ragged one of eight lanes, two empty
    hist = oracle_runs
    xe, se, ste = hist[-1]
    STALL, ENG = K["FB_S_STALL"], K["FB_S_ENG_STATE"]
    live = st0 == 0
    a = 6378137.0
    h = x0[K["FB_X_H_E"]]
    h_gp = (h - 110.0) * a / (a + h - 110.0)                          # (the geoid is within ±107 m of the ellipsoid)
    cleared = live & (s0[STALL] == 1) & (hist[1][1][STALL] == 0)      # f_step! modifies SOME lanes of a pair at the first step: k1 again for a subset
    qn = lambda x, r: np.sqrt((x[K[r]:K[r] + 4] ** 2).sum(0))
    off_unit = live & (np.abs(qn(x0, "FB_X_Q_WB") - 1) > 1e-8) & (np.abs(qn(x0, "FB_X_Q_EW") - 1) > 1e-8)
    renormed = off_unit & (np.abs(qn(hist[1][0], "FB_X_Q_WB") - 1) < 1e-12)
    # within 10 m of the terrain (h_terrain = 0: the geoid) in the middle of a launch: above it at the start, first below it in step m (1-based)
    Ng = geoid(oracle, pinned["lat"], pinned["lon"])
    clr = np.array([hk[0][K["FB_X_H_E"]] - Ng for hk in hist])
    sinks = live & (clr[0] > 10.0) & (clr[-1] < 10.0)
    m = np.where(sinks, (clr <= 10.0).argmax(0), 0)
    mid = sinks & ((m - 1) % 7 != 0) & ((m - 1) % 2 != 0)             # the launches of 7 and of 2 steps have completed a step before it
    running = [p for p in range(n // 64 + 1) if p not in (DEAD_PAIR, SINK_PAIR)]
    assert running == [0, 1, 4, 5] and (pair == 5).sum() == 8
    for p in running:
        here = (pair == p) & live
        assert (here & (h_gp > 11000.0)).any() and (here & (h < 10000.0)).any(), ("stratosphere beside troposphere", p)
        assert set(np.unique(s0[ENG, here]).tolist()) == {0, 1, 2}, ("engines off, starting, running", p)
        assert 0 < (here & (cleared | renormed)).sum() < here.sum(), ("k1 evaluated again for a part of the pair", p)
        assert (here & mid).any() and not (here & sinks).all(), ("a lane handed over while its pair goes on", p)
    assert (st0[pair == DEAD_PAIR] != 0).all() and (st0[pair != DEAD_PAIR] == 0).all()    # a pair that never runs; nobody else is terminated
    gone = pair == SINK_PAIR
    assert gone.sum() == 64 and sinks[gone].all() and len(CROSS_AT) == 3                  # the pair that leaves: every lane of it is handed over, ...
    last = int(m[gone].max())
    assert last < NSTEPS and (last - 1) % 7 != 0 and (last - 1) % 2 != 0                  # ... the last of them in the middle of a launch of 7 and of 2
    assert len(np.unique(m[gone])) >= 3                                                   # (and not all at once: the pair thins out first)
    assert (ste[live] == 0).all()                                                         # nobody ends within the run
    assert (kind[gone] == 7).all()


@pytest.mark.parametrize("spl", PARTITIONS)
def test_bit_identical_to_the_recorded_parent_build(pinned, device_runs, spl):
    (x, s, st), (x2, s2, st2), _ = device_runs[spl]
    gx, gs, gst = (pinned[f"spl{spl}_{k}"] for k in ("x", "s", "status"))
    dx = x != gx
    print("%d steps per launch: differing state words: %d of %d (rows %s, lanes %s)" % (spl, int(dx.sum()), dx.size, np.nonzero(dx.any(1))[0].tolist(),
                                                                                       np.nonzero(dx.any(0))[0].tolist()[:16]))
    assert np.array_equal(st, gst) and np.array_equal(s, gs)
    assert np.array_equal(x.view(np.uint64), gx.view(np.uint64))      # byte for byte: the sign of a zero counts
    assert np.array_equal(st2, st) and np.array_equal(s2, s) and np.array_equal(x2.view(np.uint64), x.view(np.uint64))   # and the same bytes again


@pytest.mark.parametrize("spl", PARTITIONS)
def test_agrees_with_the_one_wave_stepper_and_the_oracle(fb, pinned, oracle_runs, device_runs, spl):
    x0, s0, u, ui, st0 = _inputs(pinned)
    (x, s, st), _, (xa, sa, sta) = device_runs[spl]
    xo, so, sto = oracle_runs[NSTEPS]
    NAN = fb.K["FB_ST_NAN"]
    e_air = float((np.abs(x - xa) / np.maximum(np.abs(xa), 1e-3)).max())
    e_orc = float((np.abs(x - xo) / np.maximum(np.abs(xo), 1e-3)).max())
    print("%d steps per launch: max scaled difference after %d steps: vs the one-wave stepper %.2e, vs the oracle %.2e; status words %s"
          % (spl, NSTEPS, e_air, e_orc, np.unique(st).tolist()))
    assert not ((st & NAN != 0) & (sta & NAN == 0)).any()               # no wait ran into its bound
    assert np.array_equal(st, sta) and np.array_equal(s, sa) and np.array_equal(st, sto) and np.array_equal(s, so)
    dead = st0 != 0
    assert np.array_equal(x[:, dead], x0[:, dead])                      # terminated before the launch: untouched
    assert e_air < 1e-10
    assert e_orc < 1e-9
