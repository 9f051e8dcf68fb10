"""Cessna172Xv2 through the 10 m band of the air / ground hand-over, at 1, 7 and 50 steps per launch, on both airborne steppers, at
Δt = dt and Δt = 2 dt — every aircraft against the oracle.

The stepping kernels carry per-lane state across two boundaries: from one launch to the next, and from the airborne pass to the
ground-capable pass, which redoes a handed-over lane's whole launch from the launch-start state. What this file holds them to:

    * ctl_bak, the launch-start copy of the control-law record (cs | cu) that a handed-over lane is put back to — taken and restored
      for launches of more than one step only (csrc/c172_kernels.hpp, k_step_air: a one-step launch's only control update comes after
      its last evaluation, so a lane handed over in it has had none);
    * k1 / k1_valid, the derivative the ground-capable pass carries into the next launch, which k_step_duo's epilogue invalidates when it
      commits a lane's steps (not at entry): a lane that goes ground -> air -> ground must not start from the stale one;
    * the one-wave airborne stepper (FLIGHTBATCH_DUO=0), which carries k1 through airborne launches as well.

One batch of WA aircraft, trimmed over a runway, under the autopilot, in three groups mixed within every wave:
    (a) descending into the band from 10-30 m: half level off at 5-8 m (EAS_alt), half reverse their climb-rate reference between two
        fb.step calls at step 113 (which neither 7 nor 50 divides),
    (b) holding altitude on the boundary: h_ref (an ELLIPSOIDAL altitude, compared with h_e by the laws) 10 +/- 1 m above the terrain in
        orthometric terms, mirrored about the boundary at steps 173 and 359 — these lanes change passes from launch to launch,
    (c) climbing out of the band from 4-9 m.
No aircraft touches the runway (the per-step clearance is asserted), so every lane holds the strict tolerance; ground contact and
throws are covered by tests/test_gpu_termination.py. The band crossings are counted on the oracle stepped one step at a time (chunking
does not change its result) and asserted, so that a later retune of the trims cannot quietly take the edges away.

Not covered, on purpose: a hand-over first detected at the evaluation at x_{n+1} (where `ctl_lane = ctl_now && run` in k_step_duo and
`if (run)` in k_step_air decide a one-step launch). A natural trajectory does not get there: the k4 point and x_{n+1} agree in height
to high order, so a lane that enters the band is handed over at k4 or earlier. Only a contrived state would reach it.
"""

import numpy as np
import pytest

from oracle_binding import OracleX
from support import abi_to_oracle_rows, band_scenario, digest, geoid, state_scale, stepper

pytestmark = pytest.mark.gpu

N = 1536
H_TRN = 120.0
BAND = 10.0                      # the airborne pass's clearance limit (orthometric height over the terrain)
NSTEPS = 500
S_REVERSE = 113                  # (a): the climb-rate reference of the reversing half changes sign
S_MIRROR = (173, 359)            # (b): h_ref mirrored about the band's edge
WRITES = sorted((S_REVERSE,) + S_MIRROR)


def scenario(fb, N0):
    """trim parameters, groups and control-law inputs (drawn once, the same for every case): support.band_scenario"""
    return band_scenario(fb, N0, N, H_TRN, BAND, S_REVERSE, S_MIRROR)


_ORACLE = {}   # (ratio, digest of the start state) -> oracle run with its coverage record
_DEVICE = {}   # (spl, duo, ratio) -> device result


def device_run(fb, oracle, spl, duo, ratio):
    key = (spl, duo, ratio)
    if key in _DEVICE:
        return _DEVICE[key]
    gains = fb.ctl_gains.ctl_gains_blob()
    N0 = geoid(oracle, np.zeros(1), np.zeros(1))[0]
    tp, groups, set_cu, write = scenario(fb, N0)
    with stepper(duo):
        w = fb.Cessna172Xv2World(N, gains=gains)
    w.set_params(h_terrain=H_TRN)
    sim = fb.Simulation(w, dt=0.01, Δt=0.01 * ratio, save_on=False, steps_per_launch=spl)
    fb.init(sim, tp)
    assert w.trim_success.all()
    w.cu = set_cu(w.cu)
    start = dict(x=w.x, cs=w.cs, cu=w.cu, u=w.u, ui=w.ui, s=w.s)
    done = 0
    for s_next in WRITES + [NSTEPS]:
        fb.step(sim, (s_next - done) * 0.01)
        done = s_next
        if s_next < NSTEPS:
            w.sync()
            w.cu = write(w.cu, s_next)
    w.sync()
    tstep, twhere = w.termination
    r = dict(start=start, x=w.x, cs=w.cs, cu=w.cu, s=w.s, status=w.status, tstep=tstep, twhere=twhere, groups=groups, N0=N0, tp=tp)
    w.close()
    _DEVICE[key] = r
    return r


def oracle_run(fb, oracle, ratio, dev):
    """the oracle from the device's start state, one step at a time, with the same writes at the same steps; the per-step clearance
    of every aircraft is kept to count the band crossings"""
    st = dev["start"]
    key = (ratio, digest(*(st[k] for k in ("x", "cs", "cu", "u", "ui", "s"))))
    if key in _ORACLE:
        return _ORACLE[key]
    K = fb.K
    perm = abi_to_oracle_rows(K, "x2")
    X = OracleX(oracle, fb.ctl_gains.ctl_gains_blob())
    env = oracle.default_env(h_trn=H_TRN)
    o = X.trim_init(dev["tp"].pack(N), fb.TrimState(N), env, 0.01 * ratio, threads=16)
    o["x"][perm] = st["x"]; o.update({k: st[k].copy() for k in ("cs", "cu", "u", "ui", "s")})
    o["status"] = np.zeros(N, np.int32); o["nstep"] = 0
    _, _, _, write = scenario(fb, dev["N0"])
    clr = np.empty((NSTEPS + 1, N))
    clr[0] = o["x"][20] - dev["N0"] - H_TRN
    for k in range(NSTEPS):
        if k in WRITES:
            o["cu"] = write(o["cu"], k)
        X.step_term(o, env, 0.01, ratio, 1, threads=16)
        clr[k + 1] = o["x"][20] - dev["N0"] - H_TRN
    above = clr > BAND
    flips = np.diff(above.astype(np.int8), axis=0)
    cov = dict(down=(flips == -1).sum(0), up=(flips == 1).sum(0), min_clr=clr.min(0), above=above)
    _ORACLE[key] = (o, cov)
    return o, cov


def check_coverage(cov, groups, label):
    down, up = cov["down"], cov["up"]
    gb = groups["b"]
    frac = cov["above"][:, gb].mean()
    print(f"{label}: crossed the band downward {int((down > 0).sum())}, upward {int((up > 0).sum())}, more than once "
          f"{int(((down + up) > 1).sum())}; group (b) above it {100 * frac:.0f} % of its steps; lowest clearance {cov['min_clr'].min():.2f} m")
    assert (down > 0).sum() >= 200 and (up > 0).sum() >= 200 and ((down + up) > 1).sum() >= 100, label
    assert 0.3 <= frac <= 0.7, (label, frac)
    assert cov["min_clr"].min() > 3.0, "no wheel may come near the runway (gear legs ~1.9 m)"


CASES = [(spl, duo, ratio) for ratio in (1, 2) for spl in (1, 7, 50) for duo in (True, False)]


@pytest.mark.parametrize("spl,duo,ratio", CASES, ids=[f"spl{s}-{'duo' if d else 'air'}-r{r}" for s, d, r in CASES])
def test_x2_through_the_handover_band(fb, oracle, spl, duo, ratio):
    K = fb.K
    label = f"Xv2 band, {spl} steps per launch, {'duo' if duo else 'one-wave'}, Δt = {ratio} dt"
    dev = device_run(fb, oracle, spl, duo, ratio)
    o, cov = oracle_run(fb, oracle, ratio, dev)
    check_coverage(cov, dev["groups"], label)
    perm = abi_to_oracle_rows(K, "x2")
    thrown = int((o["status"] != 0).sum())
    print(f"{label}: threw {thrown} (oracle), {int((dev['status'] != 0).sum())} (device)")
    assert np.array_equal(dev["status"], o["status"]), f"{label}: {int((dev['status'] != o['status']).sum())} status words differ"
    assert np.array_equal(dev["tstep"], o["term_step"]) and np.array_equal(dev["twhere"], o["term_where"])
    err = np.abs(dev["x"] - o["x"][perm]) / state_scale(o["x"])[perm]
    cerr = np.abs(dev["cs"] - o["cs"]) / np.maximum(np.abs(o["cs"]), 1.0)
    per = err.max(0)
    print(f"{label}: max scaled error, state {err.max():.2e} (group a {per[dev['groups']['a']].max():.2e}, b {per[dev['groups']['b']].max():.2e}, "
          f"c {per[dev['groups']['c']].max():.2e}), record {cerr.max():.2e}")
    assert err.max() < 1e-6, (label, err.max(), np.unravel_index(err.argmax(), err.shape))
    assert cerr.max() < 1e-6, (label, cerr.max(), np.unravel_index(cerr.argmax(), cerr.shape))
    assert np.array_equal(dev["cu"], o["cu"]), f"{label}: control-law inputs differ on {int((dev['cu'] != o['cu']).any(0).sum())} aircraft"
    assert np.array_equal(dev["s"], o["s"]), f"{label}: discrete states differ"
    if not duo:
        # the two airborne steppers at the same launch length: the same trajectories to rounding
        ref = device_run(fb, oracle, spl, True, ratio)
        d = (np.abs(dev["x"] - ref["x"]) / state_scale(o["x"])[perm]).max()
        dc = (np.abs(dev["cs"] - ref["cs"]) / np.maximum(np.abs(o["cs"]), 1.0)).max()
        print(f"{label}: one-wave against duo: state {d:.2e}, record {dc:.2e}")
        assert np.array_equal(dev["status"], ref["status"]) and np.array_equal(dev["s"], ref["s"])
        assert d < 1e-9 and dc < 1e-9, (label, d, dc)
