"""fbf::k_step_f32 (csrc/c172_kernels_f32.hpp) held to the oracle through what a stepper of its own can get wrong: stall flags that flip,
engines that start, stop and run dry, k1 evaluated again for the lanes f_step! modified while their wave neighbours sit out, launches of 1, 2,
7 and 14 steps, ragged waves in one and two workgroups, lanes terminated before the launch, lanes handed over in the middle of a launch and
lanes the kernel never commits. The batch is tests/f32_cases.py's; tests/test_f32_cases_host.py shows, from the oracle alone, that no event of
it can legitimately move by a step in fp32 — so the DISCRETE history of every lane must be the oracle's, step for step.

The CONTINUOUS rows are held to a measured envelope, not to a hand-set tolerance: E = |oracle' - oracle| with the sixteen fp32-held rows of
oracle' moved by one fp32 ulp after every step; the kernel must stay within 10 x E per lane (the family's factor: it stands for the rounding
of intermediates, which a jitter of the stored state does not model), no floor. bench.F32_TOLERANCE, a stated 1000-step bound, is a ceiling
on top of that.

No two partitions of a run give the same bits, and none is asked for: q_wb is renormalised silently at f_step!, after the k1 of the next step
was formed from the unnormalised value, and a launch boundary forms that k1 afresh from the normalised one — so fused and one-step launches
differ at the fp32 ulp level, every step; a handed-over lane is redone in fp64 from the start of its launch, which a longer launch moves
earlier. Their difference is held to the same per-lane bound as the distance from the oracle.

Measured on an MI355X (this file's printout; docs/design/k_step_air.md, "fp32: what is held where"): |gpu - oracle| / E per lane, median / 90 % /
max: 0.30 / 0.64 / 1.51 after 14 steps in every partition, 0.17 / 0.46 / 1.22 after 100; no event a step away from the oracle's; no crash step off
by one. profiles/f32_defect_builds.txt: what this file sees of three defect builds of the kernel, and the one it cannot see."""
import os
import sys

import numpy as np
import pytest

import f32_cases as fc
from conditioning import check_against_envelope

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import F32_TOLERANCE   # noqa: E402

pytestmark = pytest.mark.gpu

_RUNS = {}
ROW_BOUNDS = (("rates_rad_s", slice(21, 24)), ("velocity_m_s", slice(24, 27)), ("altitude_m", slice(20, 21)), ("q_wb", slice(12, 16)),
              ("q_ew", slice(16, 20)), ("engine_speed_rad_s", slice(9, 10)))


def device_run(fb, oracle, n, nsteps, spl):
    """the FB_F32 handle's run of a size, length and partition, read after every launch (computed once, shared, left unchanged)"""
    if (n, nsteps, spl) not in _RUNS:
        _RUNS[n, nsteps, spl] = fc.run_device(fb, fc.make_inputs(fb.K, oracle, n), nsteps, spl, dtype="f32", every_launch=True)
    return _RUNS[n, nsteps, spl]


def check_discrete(fb, oracle, n, nsteps, spl, lanes):
    h, r = fc.history(fb.K, oracle, n, nsteps), device_run(fb, oracle, n, nsteps, spl)
    at = np.minimum(np.arange(0, nsteps + spl, spl), nsteps)                       # the steps completed at the launch boundaries
    assert r["hist_s"].shape[0] == at.size
    ds = (r["hist_s"] != h["s"][at]).any(1)[:, lanes]; dst = (r["hist_status"] != h["status"][at])[:, lanes]
    print("n = %d, %d steps in launches of %d: s differs from the oracle's on %d lanes, the status word on %d (of %d lanes, %d boundaries)"
          % (n, nsteps, spl, int(ds.any(0).sum()), int(dst.any(0).sum()), int(np.count_nonzero(lanes)), at.size))
    assert not ds.any(), ("s", np.flatnonzero(lanes)[ds.any(0)][:8], at[ds.any(1)][:8])
    assert not dst.any(), ("status", np.flatnonzero(lanes)[dst.any(0)][:8], at[dst.any(1)][:8])
    return h, r


def check_continuous(fb, oracle, n, nsteps, spl, label):
    K = fb.K
    inp, h, r = fc.make_inputs(K, oracle, n), fc.history(K, oracle, n, nsteps), device_run(fb, oracle, n, nsteps, spl)
    dead, airborne, banded = fc.lane_sets(K, inp, h)
    E = fc.envelope(K, oracle, n, nsteps)
    xo = h["x"][nsteps]
    err = fc.scaled_error(r["x"], xo)
    ratio = err[airborne] / E.max(0)[airborne]
    print("%s: |gpu - oracle| / envelope over the %d airborne lanes: median %.2f, 90 %% %.2f, max %.2f (lane %d, kind %d)"
          % (label, int(airborne.sum()), np.median(ratio), np.quantile(ratio, 0.9), ratio.max(), np.flatnonzero(airborne)[ratio.argmax()],
             inp["kind"][np.flatnonzero(airborne)[ratio.argmax()]]))
    check_against_envelope(err[airborne], E[:, airborne], label, floor=0.0, factor=fc.FACTOR)
    d = np.abs(r["x"] - xo)[:, airborne]
    for name, rows in ROW_BOUNDS:
        print("%s: %s %.2e (stated bound %.0e)" % (label, name, d[rows].max(), F32_TOLERANCE[name]))
        assert d[rows].max() < F32_TOLERANCE[name], (label, name)


@pytest.mark.parametrize("spl", fc.PARTITIONS[14])
@pytest.mark.parametrize("n", fc.SIZES)
def test_discrete_history_is_the_oracles(fb, oracle, n, spl):
    """s and the status word of EVERY lane at every launch boundary; with one step per launch that is the whole history, and the steps at which
    the events fall are compared themselves. Lanes terminated before the launch keep x, s, status and termination record bit for bit."""
    K = fb.K
    h, r = check_discrete(fb, oracle, n, 14, spl, np.ones(n, bool))
    inp = fc.make_inputs(K, oracle, n)
    if spl == 1:
        for name, row, val in (("stall flag set", K["FB_S_STALL"], 1), ("stall flag cleared", K["FB_S_STALL"], 0), ("engine off", K["FB_S_ENG_STATE"], 0),
                               ("engine starting", K["FB_S_ENG_STATE"], 1), ("engine running", K["FB_S_ENG_STATE"], 2)):
            want, got = fc.first_step(h["s"][:, row] == val), fc.first_step(r["hist_s"][:, row] == val)
            moved = want != got
            print("n = %d: %s: %d lanes with the event behind the start, %d at another step than the oracle's" % (n, name, int((want > 0).sum()), int(moved.sum())))
            assert not moved.any(), (name, np.flatnonzero(moved)[:8], want[moved][:8], got[moved][:8])
    dead = inp["st0"] != 0
    assert dead.any() and np.array_equal(r["x"][:, dead].view(np.uint64), inp["x0"][:, dead].view(np.uint64)) and np.array_equal(r["s"][:, dead], inp["s0"][:, dead])
    assert np.array_equal(r["status"][dead], inp["st0"][dead]) and (r["term_step"][dead] == -1).all() and (r["term_where"][dead] == K["FB_TERM_NONE"]).all()
    assert np.array_equal(r["term_step"], h["term_step"]) and np.array_equal(r["term_where"], h["term_where"])      # nobody ends within the run


@pytest.mark.parametrize("spl", fc.PARTITIONS[14])
@pytest.mark.parametrize("n", fc.SIZES)
def test_continuous_rows_within_the_envelope(fb, oracle, n, spl):
    check_continuous(fb, oracle, n, 14, spl, "n = %d, 14 steps in launches of %d" % (n, spl))


@pytest.mark.parametrize("n", fc.SIZES)
def test_partitions_differ_within_the_same_bound(fb, oracle, n):
    """Two partitions of the same run are not the same bits (module docstring: the silent q_wb renormalisation, the fp64 redo from the launch
    start); every lane's difference is held to the bound its distance from the oracle is held to."""
    E = fc.envelope(fb.K, oracle, n, 14)
    live = fc.make_inputs(fb.K, oracle, n)["st0"] == 0
    for a, b in ((1, 14), (2, 14), (7, 14), (1, 7), (1, 2), (2, 7)):
        ra, rb = device_run(fb, oracle, n, 14, a), device_run(fb, oracle, n, 14, b)
        words = ra["x"].view(np.uint64) != rb["x"].view(np.uint64)
        print("n = %d: launches of %d against launches of %d: %d of %d state words differ, on %d lanes" % (n, a, b, int(words.sum()), words.size, int(words.any(0).sum())))
        assert np.array_equal(ra["s"], rb["s"]) and np.array_equal(ra["status"], rb["status"])
        check_against_envelope(fc.scaled_error(ra["x"], rb["x"])[live], E[:, live], "n = %d: %d against %d steps per launch" % (n, a, b), floor=0.0, factor=fc.FACTOR)


@pytest.mark.parametrize("spl", fc.PARTITIONS[100])
@pytest.mark.parametrize("n", fc.SIZES)
def test_hundred_steps(fb, oracle, n, spl):
    """100 steps at 50 and at 7 per launch: the same discrete and continuous checks on the lanes the oracle keeps alive; the sinking lanes (kind
    7) fly on in fp64 after their hand-over and crash: status as the oracle's, step within one of it (their first steps were fp32 ones)."""
    K = fb.K
    inp, h = fc.make_inputs(K, oracle, n), fc.history(K, oracle, n, 100)
    alive = h["status"][-1] == 0
    h, r = check_discrete(fb, oracle, n, 100, spl, alive | (inp["st0"] != 0))
    check_continuous(fb, oracle, n, 100, spl, "n = %d, 100 steps in launches of %d" % (n, spl))
    crashed = ~alive & (inp["st0"] == 0)
    assert crashed.any() and np.array_equal(crashed, inp["kind"] == 7)
    off = r["term_step"][crashed] - h["term_step"][crashed]
    print("n = %d, 100 steps in launches of %d: %d lanes crash, termination step off by one on %d, place differs on %d"
          % (n, spl, int(crashed.sum()), int((off != 0).sum()), int((r["term_where"][crashed] != h["term_where"][crashed]).sum())))
    assert np.array_equal(r["status"][crashed], h["status"][-1][crashed]) and (np.abs(off) <= 1).all()
    assert (r["term_step"][alive] == -1).all()
