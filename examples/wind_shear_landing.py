#!/usr/bin/env python3
"""The reference's scripted crosswind landing (lib/FlightApps/demos/c172_demos.jl:406-497) with the WIND set by the script, as the demo does it: its
callback writes `world.atmosphere.wind.u.E = 6` on every call (:427-433). Here every aircraft of a Cessna172Xv2 batch flies the final leg in its own
crosswind (a parameter row), and meets a shear at its own height above the runway (a second row), below which the crosswind steps to a third row's
value — a gust front on short final, N of them at once, each simulation in its own world (per-aircraft environment rows, BatchedWorld.set_env).

The script is a scenario table (flightbatch.scenario) whose actions write the aircraft's wind rows: `mode="device"` interprets it on the device
between the stepping launches, nothing crossing to the host during the run; `mode="callback"` interprets the SAME table on the host after every
step (scenario.host_callback: inputs, control-law rows and environment rows cross PCIe both ways). Both end in the same bits.
examples/crosswind_landing.py is the demo with a constant wind; `python examples/wind_shear_landing.py [n] [device|callback]` prints a summary."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402
from flightbatch.guidance import Segment  # noqa: E402

LOC = (np.deg2rad(47.80433), np.deg2rad(12.997)); H_ORTH = 427.2; PSI = np.deg2rad(157.0)   # c172_demos.jl:17-19
# parameter rows: 0-2 / 3-5 the final leg's end points, 6 approach EAS, 7 the runway's ellipsoidal altitude, 8 the starting distance,
# 9 the crosswind (from the east) on the final leg, 10 the ellipsoidal altitude of the shear, 11 the crosswind below it
P_CW, P_H_SHEAR, P_CW_LOW = 9, 10, 11
# record rows: 0 touchdown time, 1 distance past the threshold, 2 cross-track error at touchdown, 3 the time the shear was met
PHASES = ("init", "final", "below the shear", "flare", "ground")


def scenario_table():
    from flightbatch import scenario as sc
    scn = sc.Scenario(n_par=12, n_rec=4)
    INIT, FINAL, LOW, FLARE, GROUND = (scn.phase(p) for p in PHASES)
    scn.when(INIT, sc.ALWAYS, [sc.cu("GDC_MODE_REQ", float(fb.ModeGuidance.segment))] + sc.target(0, 3) +
             [sc.cu("SEG_HOR_REQ", 1), sc.cu("SEG_VRT_REQ", 1), sc.cu("EAS_REF", sc.par(6)), sc.u("FLAPS", 1.0), sc.env("WIND_E", sc.par(P_CW))], then=FINAL)
    # atmosphere.wind.u.E = ... on every call, like the demo (an assignment of what is there already writes nothing)
    scn.always(FINAL, [sc.env("WIND_E", sc.par(P_CW))])
    for p in (LOW, FLARE, GROUND):
        scn.always(p, [sc.env("WIND_E", sc.par(P_CW_LOW))])
    scn.when(FINAL, sc.src.H_E - sc.par(P_H_SHEAR) < 0.0, [sc.env("WIND_E", sc.par(P_CW_LOW)), sc.rec(3, sc.src.T)], then=LOW)
    flare = [sc.cu("SEG_VRT_REQ", 0), sc.cu("LON_MODE_REQ", float(fb.ModeControlLon.EAS_clm)), sc.cu("CLM_REF", -0.3),
             sc.cu("LAT_MODE_REQ", float(fb.ModeControlLat.φ_β)),
             sc.cu("BETA_REF", sc.wrap_to_pi(sc.src.PSI - sc.cs_("SEG_CHI_REF") + sc.cs_("SEG_DCHI"))),   # wrap_to_π(ψ - χ_12)
             sc.cu("PHI_REF", 0.0)]
    scn.when(LOW, sc.src.H_E - sc.par(7) < 6.0, flare, then=FLARE)   # vehicle.y.kinematics.h_e - final_leg.p2.h < 6
    scn.when(FLARE, sc.src.ON_GND > 0.5, [sc.cu("THROTTLE_AXIS", 0.0), sc.cu("RUDDER_AXIS", -0.04), sc.u("FLAPS", 0.0),
                                           sc.rec(0, sc.src.T), sc.rec(1, sc.cs_("SEG_S_1B") - sc.par(8)), sc.rec(2, sc.cs_("SEG_E_SB"))], then=GROUND)
    scn.always(GROUND, [sc.cu("THROTTLE_AXIS", 0.0), sc.u("BRAKE_LEFT", 1.0), sc.u("BRAKE_RIGHT", 1.0)])
    return scn


def run(n=64, t_end=150.0, dt=0.02, seed=0, verbose=False, mode="device", every=1, s0_range=(2500.0, 3500.0), crosswind=None, shear=None, shear_height=None):
    """crosswind [n]: the east wind on the final leg (default: 2 .. 5 m/s); shear [n]: what is added to it below the shear (default: 0 .. 6 m/s);
    shear_height [n]: the height of the shear above the runway, more than the 6 m of the flare (default: 10 .. 30 m)."""
    from flightbatch import scenario as sc
    K = fb.K
    rng = np.random.default_rng(seed)
    w = fb.Cessna172Xv2World(n)
    w.set_params(h_terrain=H_ORTH)                                   # HorizontalTerrain(h_LOWS15)
    w.set_env()                                                      # every simulation's own world: rows that repeat the block (still air) until the script sets the wind
    probe = fb.TrimParameters(n_e=np.array([np.cos(LOC[0]) * np.cos(LOC[1]), np.cos(LOC[0]) * np.sin(LOC[1]), np.sin(LOC[0])]), h_e=1000.0)
    sim = fb.Simulation(w, dt=dt, Δt=dt, save_on=False, steps_per_launch=1)
    fb.init(sim, probe)
    fb.f_ode(w)
    y = w.y
    geoid = float((y[K["FB_Y_KIN"] + 20] - y[K["FB_Y_KIN"] + 21])[0])
    p_rwy = np.array([LOC[0], LOC[1], H_ORTH + geoid])
    s0 = rng.uniform(s0_range[0], s0_range[1], n)
    p2 = np.repeat(p_rwy[:, None], n, axis=1)
    far = Segment.from_origin(p2, s0, PSI + np.pi, γ=np.deg2rad(3)).p2
    EAS = rng.uniform(29.0, 32.0, n)
    cw = rng.uniform(2.0, 5.0, n) if crosswind is None else np.asarray(crosswind, dtype=np.float64).reshape(n)
    dcw = rng.uniform(0.0, 6.0, n) if shear is None else np.asarray(shear, dtype=np.float64).reshape(n)
    h_sh = rng.uniform(10.0, 30.0, n) if shear_height is None else np.asarray(shear_height, dtype=np.float64).reshape(n)
    n_e = np.array([np.cos(far[0]) * np.cos(far[1]), np.cos(far[0]) * np.sin(far[1]), np.sin(far[0])])
    fb.init(sim, fb.TrimParameters(n_e=n_e, h_e=far[2], EAS=EAS, ψ_nb=PSI, γ_wb_n=-np.deg2rad(3), flaps=1.0, fuel_load=0.5))
    assert w.trim_success.all(), "approach trim failed"
    par = np.concatenate([far, p2, EAS[None], np.full((1, n), p_rwy[2]), s0[None], cw[None], (p_rwy[2] + h_sh)[None], (cw + dcw)[None]])
    scn = scenario_table()
    if mode == "device":
        w.set_scenario(scn, params=par, every=every, rec_init=np.nan)
        sim = fb.Simulation(w, dt=dt, Δt=dt, save_on=False, steps_per_launch=50)
        fb.step(sim, t_end); w.sync()
        st = w.scenario_state()
        phase, since, rec = st["phase"].astype(int), st["since"], st["rec"]
    else:
        st = dict(phase=np.zeros(n, np.int64), since=np.zeros(n, np.int64), step=0, par=par.copy(), rec=np.full((scn.n_rec, n), np.nan))
        sim = fb.Simulation(w, dt=dt, Δt=dt, save_on=False, user_callback=sc.host_callback(scn.pack(), st, dt, every=every))
        fb.step(sim, t_end); w.sync()
        phase, since, rec = st["phase"].astype(int), st["since"], st["rec"]
    out = dict(phase=phase, since=since, rec=rec, status=w.status, x=w.x, s=w.s, u=w.u, ui=w.ui, cu=w.cu, cs=w.cs, env=w.env, crosswind=cw, shear=dcw, shear_height=h_sh)
    if verbose:
        print(f"n = {n} ({mode}): phases {np.bincount(phase, minlength=5)}, terminated {int((out['status'] != 0).sum())}, shear met at "
              f"{np.nanmin(rec[3]):.1f}-{np.nanmax(rec[3]):.1f} s, touchdown at {np.nanmin(rec[0]):.1f}-{np.nanmax(rec[0]):.1f} s")
        for lo in (0.0, 2.0, 4.0):
            m = (dcw >= lo) & (dcw < lo + 2.0) & np.isfinite(rec[2])
            if m.any():
                print(f"shear {lo:.0f}-{lo + 2:.0f} m/s: {int(m.sum())} aircraft, cross-track at touchdown {np.abs(rec[2][m]).mean():.2f} m (mean of |e|), max {np.abs(rec[2][m]).max():.2f} m")
    w.close()
    return out


if __name__ == "__main__":
    n_ = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    run(n_, verbose=True, mode="callback" if "callback" in sys.argv[2:] else "device")
