#!/usr/bin/env python3
"""Generates tests/golden/duo_waits_pin_parent.npz ON THE GPU, from the library that is built in the tree: a DEVICE-GENERATED fixture.

It pins k_step_duo<WA>'s results bit for bit (tests/test_gpu_duo_waits.py) across a change of how the two waves of a pair wait for each
other (duo_wait / duo_publish, c172_kernels.hpp). A wrong wait shows as a stale hand-over — wrong bits — or as FB_ST_NAN from a wait that
ran into its bound, so the batch makes the two roles arrive at their points in every order. Record it with the build the change starts
from, commit it with the change; regenerate it whenever a later change MEANS to alter rounding (and say so in that change).

n = 328: workgroup 0 with four full wave pairs, workgroup 1 with a full pair, a ragged one of eight lanes and two empty ones. 14 steps of
0.01 s, run three times: in launches of 1, 2 and 7 steps. The inputs come from the CPU oracle's trim (make_duo_stage_pin.py's recipe).
Pair 2 (lanes 128-191) is terminated before the launch, every lane of it: both waves only publish. Pair 3 (lanes 192-255) sinks through
10 m of clearance over the terrain, every lane of it, the last ones in step 12: the pair leaves in the middle of a launch (EXIT word).
In the other pairs lane k is of kind k % 8:

    0  cruise; every other one in the stratosphere (role P's longer atmosphere branch: role D waits at A and W)
    1  stall flag set at a cruise angle of attack: the first f_step! clears it, k1 is evaluated again for these lanes of the pair alone
    2  attitude quaternions off unit norm at the start: the first f_step! renormalises them (and k1 is evaluated again)
    3  cruise, manual mixture
    4  engine starting, a few rad/s below idle speed: running within the run
    5  engine off, windmilling
    6  cruise in the stratosphere
    7  sinking through 10 m of clearance in the middle of a launch: handed over while its pair goes on

    python tests/golden/make_duo_waits_pin.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_duo_stage_pin as sp  # noqa: E402

OUT = os.path.join(HERE, "duo_waits_pin_parent.npz")
N, NSTEPS, PARTITIONS, DT = 328, sp.NSTEPS, (1, 2, 7), sp.DT
DEAD_PAIR, SINK_PAIR = 2, 3
SINK = 12.0                         # sink rate of the lanes that cross [m/s]
CROSS_AT = (3.5, 9.5, 11.5)         # the steps after which their clearance reaches 10 m (by turns)


def kinds(n=N):
    """the kind of every lane: k % 8, -1 in the pair terminated before the launch, 7 in the pair that leaves"""
    k = np.arange(n)
    kind = k % 8
    kind[k // 64 == DEAD_PAIR] = -1
    kind[k // 64 == SINK_PAIR] = 7
    return kind


def make_inputs(K, orc, n=N):
    """x0, s0, u, ui, status0 and the lanes' latitude / longitude (for the geoid under them)"""
    rng = np.random.default_rng(20261021 + n)
    tp = np.zeros((K["FB_NTP"], n))
    tp[K["FB_TP_N_E"]] = 1.0; tp[K["FB_TP_H_E"]] = 1000.0; tp[K["FB_TP_EAS"]] = rng.uniform(40.0, 55.0, n)
    tp[K["FB_TP_PSI_NB"]] = rng.uniform(-np.pi, np.pi, n)
    tp[K["FB_TP_FUEL_LOAD"]] = 0.5; tp[K["FB_TP_MIXTURE"]] = 0.5
    tp[K["FB_TP_PAYLOAD"]:K["FB_TP_PAYLOAD"] + 5] = np.array([75.0, 75.0, 0.0, 0.0, 50.0])[:, None]
    ts = np.tile(np.array([[0.08], [0.0], [0.75], [0.4], [0.0], [0.0], [0.0]]), (1, n))
    r = orc.trim(tp, ts, orc.default_env())
    assert r["ok"].all()
    x, s, u, ui = r["x"].copy(), r["s"].copy(), r["u"].copy(), r["ui"].copy()
    kind = kinds(n)
    k = np.arange(n)
    QWB, QEW, HE, OM, VB = (K[q] for q in ("FB_X_Q_WB", "FB_X_Q_EW", "FB_X_H_E", "FB_X_OMEGA_EB_B", "FB_X_V_EB_B"))
    lat, lon = rng.uniform(-1.4, 1.4, n), rng.uniform(-np.pi, np.pi, n)
    x[QEW:QEW + 4] = sp._q_ew(lat, lon)
    high = (kind == 6) | ((kind == 0) & ((k // 8) % 2 == 0))          # above 11 km of geopotential altitude, in every pair that runs
    x[HE] = np.where(high, rng.uniform(11500.0, 16000.0, n), rng.uniform(300.0, 4000.0, n))
    x[OM:OM + 3] += rng.normal(0, 0.02, (3, n))                       # not a steady state
    u[K["FB_U_THROTTLE"]] = rng.uniform(0.1, 1.0, n)
    u[K["FB_U_MIXTURE"]] = rng.uniform(0.2, 1.0, n)
    s[K["FB_S_STALL"], kind == 1] = 1
    x[QWB:QWB + 4, kind == 2] *= 1 + 4e-8
    x[QEW:QEW + 4, kind == 2] *= 1 - 3e-8
    ui[kind == 3] &= ~np.int32(K["FB_UI_MIXTURE_AUTO"])
    s[K["FB_S_ENG_STATE"], kind == 4] = 1
    ui[kind == 4] |= K["FB_UI_ENG_START"]
    x[K["FB_X_ENG_OMEGA"], kind == 4] = 600 * np.pi / 30 - rng.uniform(20.0, 30.0, int((kind == 4).sum()))
    u[K["FB_U_THROTTLE"], kind == 4] = 0.3
    s[K["FB_S_ENG_STATE"], kind == 5] = 0
    st0 = np.zeros(n, np.int32)
    st0[kind == -1] = K["FB_ST_NAN"]
    k7 = np.nonzero(kind == 7)[0]
    V = np.sqrt((x[VB:VB + 3] ** 2).sum(0))
    dth = -np.arcsin(SINK / V[k7])
    z = np.zeros(k7.size)
    x[QWB:QWB + 4, k7] = sp._qmul(x[QWB:QWB + 4, k7], np.stack([np.cos(dth / 2), z, np.sin(dth / 2), z]))
    x[HE, k7] = sp.geoid(orc, lat[k7], lon[k7]) + 10.0 + SINK * DT * np.array(CROSS_AT)[np.arange(k7.size) % len(CROSS_AT)]
    return x, s, u, ui, st0, lat, lon


def run(fb, x, s, u, ui, st0, spl, duo=True):
    return sp.run(fb, x, s, u, ui, st0, spl, duo=duo)


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import flightbatch as fb
    orc = sp._oracle()
    x0, s0, u, ui, st0, lat, lon = make_inputs(fb.K, orc)
    rec = dict(generated_by="device (k_step_duo<WA>), tests/golden/make_duo_waits_pin.py", dt=DT, nsteps=NSTEPS, partitions=np.array(PARTITIONS),
               x0=x0, s0=s0, u=u, ui=ui, status0=st0, lat=lat, lon=lon)
    for spl in PARTITIONS:
        x, s, st = run(fb, x0, s0, u, ui, st0, spl)
        x2, s2, st2 = run(fb, x0, s0, u, ui, st0, spl)
        assert np.array_equal(x, x2) and np.array_equal(s, s2) and np.array_equal(st, st2), "the stepper is not deterministic run to run"
        rec.update({f"spl{spl}_x": x, f"spl{spl}_s": s, f"spl{spl}_status": st})
        print("%d steps per launch: status words %s" % (spl, np.unique(st).tolist()))
    np.savez_compressed(OUT, **rec)
    print("written:", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
