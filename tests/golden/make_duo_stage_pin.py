#!/usr/bin/env python3
"""Generates tests/golden/duo_stage_pin_parent.npz ON THE GPU, from the library that is built in the tree: a DEVICE-GENERATED fixture.

It pins k_step_duo<WA>'s results bit for bit (tests/test_gpu_duo_stage_emit.py) across a change of the row emit that puts the RK stage
behind a scalar branch: what such a branch can break is the evaluation that closes a launch (stage 3 as the last one), a launch that
opens on zeroed stage sums, and a k1 that is evaluated again for some lanes of a pair only. Record it with the build the change starts
from, commit it with the change; regenerate it whenever a later change MEANS to alter rounding (and say so in that change).

Two batches: n = 72 (one workgroup: a full wave pair, a ragged one of eight lanes, two empty) and n = 264 (a second workgroup), 14 steps
of 0.01 s, run three times: in launches of 1, 2 and 7 steps. The inputs come from the CPU oracle's trim, so they can be formed without
a GPU; lane k is of kind k % 8:

    0  ordinary cruise
    1  stall flag set at a cruise angle of attack: the first f_step! clears it, k1 is evaluated again for these lanes of the pair alone
    2  attitude quaternions off unit norm by 4e-8 / 3e-8 at the start: the first f_step! renormalises them (and k1 is evaluated again)
    3  pitching up through alpha_stall_hi within the run
    4  engine starting, a few rad/s below idle speed: running within the run
    5  engine off, windmilling: no fuel flow, the fuel row's derivative is -0.0
    6  terminated before the launch (every other one; the rest cruise in the stratosphere)
    7  sinking through 10 m of clearance over the terrain (h_terrain = 0: over the geoid) in the middle of a launch: handed over

    python tests/golden/make_duo_stage_pin.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "duo_stage_pin_parent.npz")
SIZES, NSTEPS, PARTITIONS, DT = (72, 264), 14, (1, 2, 7), 0.01
ALPHA0, PITCH_RATE = 0.33, 1.6          # kind 3: angle of attack and pitch rate at the start
SINK, CROSS_AT = 12.0, (3.5, 11.5)       # kind 7: sink rate [m/s]; the steps after which the clearance reaches 10 m (alternating)
_D = C.POINTER(C.c_double)


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_binding import Oracle
    return Oracle()


def _qmul(a, b):
    return np.stack([a[0]*b[0]-a[1]*b[1]-a[2]*b[2]-a[3]*b[3], a[0]*b[1]+a[1]*b[0]+a[2]*b[3]-a[3]*b[2],
                     a[0]*b[2]-a[1]*b[3]+a[2]*b[0]+a[3]*b[1], a[0]*b[3]+a[1]*b[2]-a[2]*b[1]+a[3]*b[0]])


def _q_ew(lat, lon):
    """q_ew = Rz(lon) ∘ Ry(-(lat + π/2)), wander angle 0"""
    a = -(lat + np.pi / 2)
    cz, sz, cy, sy = np.cos(lon / 2), np.sin(lon / 2), np.cos(a / 2), np.sin(a / 2)
    return np.stack([cz * cy, -sz * sy, cz * sy, sz * cy])


def geoid(orc, lat, lon):
    out = np.zeros_like(lat)
    for k in range(lat.size):
        n_e = np.array([np.cos(lat[k]) * np.cos(lon[k]), np.cos(lat[k]) * np.sin(lon[k]), np.sin(lat[k])])
        out[k] = orc.lib.fo_geoid_height(n_e.ctypes.data_as(_D))
    return out


def make_inputs(K, orc, n):
    """x0, s0, u, ui, status0 and the lanes' latitude / longitude (for the geoid under them)"""
    rng = np.random.default_rng(20261020 + n)
    tp = np.zeros((K["FB_NTP"], n))
    tp[K["FB_TP_N_E"]] = 1.0; tp[K["FB_TP_H_E"]] = 1000.0; tp[K["FB_TP_EAS"]] = rng.uniform(40.0, 55.0, n)
    tp[K["FB_TP_PSI_NB"]] = rng.uniform(-np.pi, np.pi, n)
    tp[K["FB_TP_FUEL_LOAD"]] = 0.5; tp[K["FB_TP_MIXTURE"]] = 0.5
    tp[K["FB_TP_PAYLOAD"]:K["FB_TP_PAYLOAD"] + 5] = np.array([75.0, 75.0, 0.0, 0.0, 50.0])[:, None]
    ts = np.tile(np.array([[0.08], [0.0], [0.75], [0.4], [0.0], [0.0], [0.0]]), (1, n))
    r = orc.trim(tp, ts, orc.default_env())
    assert r["ok"].all()
    x, s, u, ui = r["x"].copy(), r["s"].copy(), r["u"].copy(), r["ui"].copy()
    kind = np.arange(n) % 8
    QWB, QEW, HE, OM, VB = (K[k] for k in ("FB_X_Q_WB", "FB_X_Q_EW", "FB_X_H_E", "FB_X_OMEGA_EB_B", "FB_X_V_EB_B"))
    lat, lon = rng.uniform(-1.4, 1.4, n), rng.uniform(-np.pi, np.pi, n)
    x[QEW:QEW + 4] = _q_ew(lat, lon)
    x[HE] = rng.uniform(300.0, 4000.0, n)
    x[OM:OM + 3] += rng.normal(0, 0.02, (3, n))                       # not a steady state
    u[K["FB_U_THROTTLE"]] = rng.uniform(0.1, 1.0, n)
    u[K["FB_U_MIXTURE"]] = rng.uniform(0.2, 1.0, n)
    # 1: the stall flag set at a cruise angle of attack
    s[K["FB_S_STALL"], kind == 1] = 1
    # 2: quaternions off unit norm
    x[QWB:QWB + 4, kind == 2] *= 1 + 4e-8
    x[QEW:QEW + 4, kind == 2] *= 1 - 3e-8
    # 3: pitching up through alpha_stall_hi
    k3 = kind == 3
    V = np.sqrt((x[VB:VB + 3] ** 2).sum(0))
    x[VB, k3] = V[k3] * np.cos(ALPHA0); x[VB + 1, k3] = 0.0; x[VB + 2, k3] = V[k3] * np.sin(ALPHA0)
    x[K["FB_X_ALPHA_FILT"], k3] = ALPHA0
    x[OM + 1, k3] = PITCH_RATE
    # 4: starting, below idle speed; 5: off, windmilling
    s[K["FB_S_ENG_STATE"], kind == 4] = 1
    ui[kind == 4] |= K["FB_UI_ENG_START"]
    x[K["FB_X_ENG_OMEGA"], kind == 4] = 600 * np.pi / 30 - rng.uniform(20.0, 30.0, int((kind == 4).sum()))
    u[K["FB_U_THROTTLE"], kind == 4] = 0.3
    s[K["FB_S_ENG_STATE"], kind == 5] = 0
    # 6: terminated before the launch, every other one; the rest in the stratosphere
    k6 = kind == 6
    dead = k6 & ((np.arange(n) // 8) % 2 == 0)
    x[HE, k6 & ~dead] = rng.uniform(11500.0, 16000.0, int((k6 & ~dead).sum()))
    st0 = np.zeros(n, np.int32)
    st0[dead] = K["FB_ST_NAN"]
    # 7: sinking through 10 m of clearance in the middle of a launch (the velocity vector pitched down, as tests/support.py's flying_batch does)
    k7 = np.nonzero(kind == 7)[0]
    dth = -np.arcsin(SINK / V[k7])
    z = np.zeros(k7.size)
    x[QWB:QWB + 4, k7] = _qmul(x[QWB:QWB + 4, k7], np.stack([np.cos(dth / 2), z, np.sin(dth / 2), z]))
    x[HE, k7] = geoid(orc, lat[k7], lon[k7]) + 10.0 + SINK * DT * np.where(np.arange(k7.size) % 2 == 0, CROSS_AT[0], CROSS_AT[1])
    return x, s, u, ui, st0, lat, lon


def run(fb, x, s, u, ui, st0, spl, duo=True):
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
    sim = fb.Simulation(w, dt=DT, save_on=False, steps_per_launch=spl)
    fb.step(sim, NSTEPS * DT); w.sync()
    out = (w.x, w.s, w.status)
    w.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import flightbatch as fb
    orc = _oracle()
    rec = dict(generated_by="device (k_step_duo<WA>), tests/golden/make_duo_stage_pin.py", dt=DT, nsteps=NSTEPS, partitions=np.array(PARTITIONS))
    for n in SIZES:
        x0, s0, u, ui, st0, lat, lon = make_inputs(fb.K, orc, n)
        rec.update({f"n{n}_x0": x0, f"n{n}_s0": s0, f"n{n}_u": u, f"n{n}_ui": ui, f"n{n}_status0": st0, f"n{n}_lat": lat, f"n{n}_lon": lon})
        for spl in PARTITIONS:
            x, s, st = run(fb, x0, s0, u, ui, st0, spl)
            x2, s2, st2 = run(fb, x0, s0, u, ui, st0, spl)
            assert np.array_equal(x, x2) and np.array_equal(s, s2) and np.array_equal(st, st2), "the stepper is not deterministic run to run"
            rec.update({f"n{n}_spl{spl}_x": x, f"n{n}_spl{spl}_s": s, f"n{n}_spl{spl}_status": st})
            print("n = %d, %d steps per launch: status words %s" % (n, spl, np.unique(st).tolist()))
    np.savez_compressed(OUT, **rec)
    print("written:", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
