"""Scenario tables on a Cessna172Sv0 batch (k_scenario_sv0, csrc/scenario_kernels.hpp): the device-side `user_callback!` of the model the
reference's first demos script (nlsim_q / nlsim_θ: one second from trim, then `act.u.elevator += 0.1`, c172_demos.jl:108-206).

Every case runs N = 300 aircraft (two workgroups, the second with 44 lanes: one partial wave) at dt = 0.02 for at most about 600 steps, with
per-aircraft parameters drawn so that the lanes of a wave sit in different phases at the same step — the ballot-gated evaluation of f_ode! and
the mixed walk are exercised only then. The host side of every bit-for-bit comparison is the SAME table run by
flightbatch.scenario.evaluate_on_host from a Simulation(user_callback=...), with fb.f_ode + mdl.y where the table reads vehicle.y."""
import io
import os
import sys

import numpy as np
import pytest

from support import (assert_same_run, lattice_trim_params, load_scenario_blob as _load, run_table_on_device, same as _same, scenario_result, state_scale,
                     table_state)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DT = 300, 0.02
KINS = ["WA", "ECEF", "NED"]


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def doublet_table():
    """memory-only (clock, inputs, parameters): an elevator doublet on u.elevator with per-aircraft switch times — parameter rows: amplitude, t1 .. t4"""
    from flightbatch import scenario as sc
    scn = sc.Scenario(n_par=5, n_rec=1)
    P = [scn.phase(p) for p in ("before", "up", "level", "down", "after")]
    elev = sc.u_("ELEVATOR")
    scn.when(P[0], sc.src.T - sc.par(1) >= 0.0, [sc.u("ELEVATOR", elev + sc.par(0))], then=P[1])
    scn.when(P[1], sc.src.T - sc.par(2) >= 0.0, [sc.u("ELEVATOR", elev - sc.par(0))], then=P[2])
    scn.when(P[2], sc.src.T - sc.par(3) >= 0.0, [sc.u("ELEVATOR", elev - sc.par(0))], then=P[3])
    scn.when(P[3], sc.src.T - sc.par(4) >= 0.0, [sc.u("ELEVATOR", elev + sc.par(0)), sc.rec(0, sc.src.T_IN_PHASE)], then=P[4])
    return scn


def doublet_params(rng, n):
    t = np.cumsum(rng.uniform(0.3, 1.4, (4, n)), axis=0)
    return np.concatenate([rng.uniform(0.03, 0.1, (1, n)), t])


PITCH_STEPS = 500


def pitch_table():
    """reads vehicle.y: an elevator step at a per-aircraft time; when θ exceeds the aircraft's threshold the elevator goes back and T, θ are
    recorded; when the climb rate turns negative (the top of the phugoid the pulse excited) the throttle is set from a parameter and EAS recorded.
    Parameter rows: amplitude, θ threshold, throttle, time of the step. The first rule reads memory only, the other two stop the walk at stage B."""
    from flightbatch import scenario as sc
    scn = sc.Scenario(n_par=4, n_rec=3)
    TRIM, PITCHING, OVER, DONE = (scn.phase(p) for p in ("trim", "pitching", "over the top", "done"))
    scn.when(TRIM, sc.src.T - sc.par(3) >= 0.0, [sc.u("ELEVATOR", sc.u_("ELEVATOR") + sc.par(0))], then=PITCHING)
    scn.when(PITCHING, sc.src.THETA - sc.par(1) > 0.0, [sc.u("ELEVATOR", sc.u_("ELEVATOR") - sc.par(0)), sc.rec(0, sc.src.T), sc.rec(1, sc.src.THETA)], then=OVER)
    scn.when(OVER, sc.src.CLM < 0.0, [sc.u("THROTTLE", sc.par(2)), sc.rec(2, sc.src.EAS)], then=DONE)
    return scn


def pitch_trim(fb, rng, n):
    return fb.TrimParameters(EAS=rng.uniform(36.0, 46.0, n), h_e=rng.uniform(500.0, 2500.0, n))


def pitch_params(rng, theta0, n):
    """(the step times are odd multiples of dt / 2: the clock rule never sits on its threshold)"""
    return np.stack([rng.uniform(0.06, 0.15, n), theta0 + rng.uniform(0.03, 0.08, n), rng.uniform(0.3, 0.9, n), (rng.integers(5, 50, n) + 0.5) * DT])


def ground_table():
    """take-off from rest: brakes off and full throttle held in every phase; at the aircraft's rotation speed the elevator comes from a parameter;
    when no strut carries weight any more the lift-off time is recorded. Parameter rows: v_r, elevator."""
    from flightbatch import scenario as sc
    scn = sc.Scenario(n_par=2, n_rec=1)
    ROLL, ROTATE, CLIMB = (scn.phase(p) for p in ("roll", "rotate", "climb"))
    for p in (ROLL, ROTATE, CLIMB):
        scn.always(p, [sc.u("BRAKE_LEFT", 0.0), sc.u("BRAKE_RIGHT", 0.0), sc.u("THROTTLE", 1.0)])
    scn.when(ROLL, sc.src.EAS - sc.par(0) > 0.0, [sc.u("ELEVATOR", sc.par(1))], then=ROTATE)
    scn.when(ROTATE, sc.src.ON_GND.eq(0.0), [sc.rec(0, sc.src.T)], then=CLIMB)
    return scn


# ---- the two ways to run a table ---------------------------------------------------------------------------------------------------------
def outputs_for_table(K, y):
    """what the table's sources name, from an output record [FB_NY, n] (the device's or the oracle's)"""
    kin, ldg = K["FB_Y_KIN"], K["FB_Y_LDG"]
    return dict(h_e=y[kin + 20], psi=y[kin], theta=y[kin + 1], phi=y[kin + 2], chi=y[kin + 38], EAS=y[K["FB_Y_AIR"] + 20], clm=-y[kin + 36],
                on_gnd=((y[ldg + 1] + y[ldg + 12] + y[ldg + 23]) > 0).astype(np.float64))


def run_callback(fb, w, scn, par, steps, reads_y):
    """the table as the host closure: after EVERY step, on the model's own arrays (and its outputs from fb.f_ode where the table reads them) — this
    file's own form of support.run_table_as_callback, which leaves the fetching to flightbatch.scenario.host_callback"""
    from flightbatch import scenario as sc
    blob = scn.pack(model="Cessna172Sv0")
    st = table_state(w.n, scn, par)

    def callback(mdl):
        st["step"] += 1
        u, ui = mdl.u, mdl.ui
        st.update(u=u, ui=ui, s=mdl.s, active=mdl.status == 0)
        if reads_y:
            fb.f_ode(mdl)
            st.update(outputs_for_table(fb.K, mdl.y))
        sc.evaluate_on_host(blob, st, st["step"] * DT, DT)
        mdl.u = u; mdl.ui = ui
    sim = fb.Simulation(w, dt=DT, save_on=False, user_callback=callback)
    fb.step(sim, steps * DT); w.sync()
    return scenario_result(w, st)


def trimmed_pair(fb, kin, tp, env_rows=False):
    """two worlds with the same device trim, and the trimmed pitch angle"""
    ws = []
    for _ in range(2):
        w = fb.BatchedWorld(N, kinematics=kin)
        if env_rows:
            w.set_env()   # per-aircraft rows that repeat the batch-wide block
        fb.f_init(w, tp)
        assert w.trim_success.all()
        ws.append(w)
    fb.f_ode(ws[0])
    theta0 = ws[0].y[fb.K["FB_Y_KIN"] + 1].copy()
    assert _same(ws[0].x, ws[1].x)
    return ws[0], ws[1], theta0


_PITCH = {}


def pitch_device_run(fb, kin="WA", spl=50, every=1, env_rows=False, steps=PITCH_STEPS):
    """case 3's table on the device (computed once per variant and shared; the results are not modified)"""
    key = (kin, spl, every, env_rows, steps)
    if key not in _PITCH:
        rng = np.random.default_rng(12)
        tp = pitch_trim(fb, rng, N)
        w = fb.BatchedWorld(N, kinematics=kin)
        if env_rows:
            w.set_env()
        fb.f_init(w, tp)
        assert w.trim_success.all()
        fb.f_ode(w)
        par = pitch_params(rng, w.y[fb.K["FB_Y_KIN"] + 1].copy(), N)
        out = run_table_on_device(fb, w, pitch_table(), par, steps, DT, spl=spl, every=every)
        out["par"] = par
        w.close()
        _PITCH[key] = out
    return _PITCH[key]


# ---- 1. acceptance and refusals -----------------------------------------------------------------------------------------------------------
def test_tables_load_on_cessna172sv0_and_what_it_lacks_is_refused(fb):
    from flightbatch import scenario as sc
    good = sc.Scenario(n_par=1, n_rec=1)
    A, B = good.phase("a"), good.phase("b")
    good.when(A, sc.src.T >= 1.0, [sc.u("ELEVATOR", sc.u_("ELEVATOR") + sc.par(0)), sc.ui("ENG_STOP", 0.0), sc.rec(0, sc.src.T)], then=B)

    def with_action(action=None, cond=None):
        scn = sc.Scenario(n_par=1, n_rec=1)
        a, b = scn.phase("a"), scn.phase("b")
        scn.when(a, cond if cond is not None else sc.src.T >= 1.0, [action] if action is not None else [], then=b)
        return scn.pack()

    bad = {"CS source": with_action(cond=sc.cs_("SEG_S_2B") > -200.0), "CU source": with_action(sc.rec(0, sc.cu_("EAS_REF"))),
           "CU destination": with_action(sc.cu("EAS_REF", sc.par(0)))}
    for kin in KINS:
        w = fb.BatchedWorld(64, kinematics=kin)
        for what, blob in bad.items():   # refused on the host, before anything is allocated: the handle stays usable, no rows exist
            assert _load(fb, w, blob) != 0 and b"Cessna172Xv2" in fb.lib.fb_last_error(), (kin, what, fb.lib.fb_last_error())
            assert fb.lib.fb_scenario_configure(w._h, 1) != 0 and b"no scenario table" in fb.lib.fb_last_error(), (kin, what)
        w.set_scenario(good, params=np.full((1, 64), 0.1))
        assert (w.scenario_state()["phase"] == 0).all()
        # the state of a Cessna172Sv0 has 27 rows on the device
        assert _load(fb, w, with_action(sc.rec(0, sc.x_(26)))) == 0
        assert _load(fb, w, with_action(sc.rec(0, sc.x_(27)))) != 0 and b"source row" in fb.lib.fb_last_error()
        assert _load(fb, w, with_action(cond=sc.x_(27) > 0.0)) != 0 and b"source row" in fb.lib.fb_last_error()
        assert _load(fb, w, good.pack()) == 0, "a rejected table must leave the handle usable"
        w.close()
    x2 = fb.Cessna172Xv2World(64)
    assert _load(fb, x2, with_action(sc.rec(0, sc.x_(27)))) == 0 and _load(fb, x2, with_action(sc.rec(0, sc.x_(33)))) == 0
    assert _load(fb, x2, with_action(sc.rec(0, sc.x_(34)))) != 0
    for blob in bad.values():
        assert _load(fb, x2, blob) == 0
    x2.close()
    f32 = fb.BatchedWorld(64, dtype="f32")
    assert _load(fb, f32, good.pack()) != 0 and b"FB_F32" in fb.lib.fb_last_error() and b"float" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError):
        f32.set_scenario(good, params=np.full((1, 64), 0.1))
    f32.close()
    r2 = fb.Robot2DWorld(64)
    assert _load(fb, r2, good.pack()) != 0 and b"another model family" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError):
        r2.set_scenario(good, params=np.full((1, 64), 0.1))
    r2.close()


# ---- 2. memory-only table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kin", KINS)
def test_memory_only_table_equals_the_host_callback(fb, kin):
    """An elevator doublet with per-aircraft switch times: no rule or action reads vehicle.y, so no wave evaluates f_ode! (stage B is skipped).
    Device table (every = 1, steps_per_launch = 50) against the same table from a host callback: x, s, u, ui, status, phase, entry step, record."""
    rng = np.random.default_rng(7)
    tp = fb.TrimParameters(EAS=rng.uniform(38.0, 52.0, N), h_e=rng.uniform(500.0, 2500.0, N), ψ_nb=rng.uniform(-3.0, 3.0, N))
    par = doublet_params(rng, N)
    wa, wb, _ = trimmed_pair(fb, kin, tp)
    steps = int(np.ceil(par[4].max() / DT)) + 20
    assert steps <= 600
    a = run_callback(fb, wa, doublet_table(), par, steps, reads_y=False)
    b = run_table_on_device(fb, wb, doublet_table(), par, steps, DT)
    mid = int(par[2].mean() / DT)
    print(f"{kin}: {steps} steps; final phases {np.bincount(b['phase'], minlength=5)}; entry steps of the last phase {b['since'].min()}..{b['since'].max()} (mean t2 at step {mid})")
    assert (b["phase"] == 4).all() and (b["status"] == 0).all() and np.unique(b["since"]).size > 20
    assert_same_run(a, b, kin)
    wa.close(); wb.close()


# ---- 3. table that reads vehicle.y, airborne -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kin", KINS)
def test_table_reading_vehicle_outputs_equals_the_host_callback(fb, kin):
    """θ and the climb rate come from the wave's one evaluation of f_ode! on the device, from fb.f_ode + mdl.y on the host; the recorded T, θ and
    EAS must be the same bits, like everything else."""
    b = pitch_device_run(fb, kin)
    rng = np.random.default_rng(12)
    tp = pitch_trim(fb, rng, N)
    w = fb.BatchedWorld(N, kinematics=kin)
    fb.f_init(w, tp)
    a = run_callback(fb, w, pitch_table(), b["par"], PITCH_STEPS, reads_y=True)
    w.close()
    print(f"{kin}: final phases {np.bincount(b['phase'], minlength=4)}; θ rule fired at steps {np.nanmin(b['rec'][0]) / DT:.0f}..{np.nanmax(b['rec'][0]) / DT:.0f}, "
          f"climb-rate rule at {b['since'].min()}..{b['since'].max()}")
    assert (b["phase"] == 3).all() and (b["status"] == 0).all() and np.isfinite(b["rec"]).all()
    assert np.unique(b["since"]).size > 20, "the aircraft must pass through their phases at different steps"
    assert _same(b["u"][fb.K["FB_U_THROTTLE"]], b["par"][2])
    assert_same_run(a, b, kin)


# ---- 4. ground table ---------------------------------------------------------------------------------------------------------------------
def test_takeoff_table_on_the_ground_equals_the_host_callback_and_lifts_off_in_order(fb, oracle):
    """From rest on the runway (set up like test_takeoff_ground_to_air_handover): brakes off, full throttle, the elevator at the aircraft's own rotation
    speed, the lift-off time recorded when ON_GND (weight on any wheel, from the ground-capable evaluation) drops to 0. The heavier aircraft rotate
    later and with less elevator (payload and elevator are monotone in v_r), so the lift-off times are ordered like v_r: asserted on the CPU oracle
    stepped with the same table first, then on the device — which also equals the host callback bit for bit."""
    from flightbatch import scenario as sc
    K = fb.K
    steps = 520
    rng = np.random.default_rng(0)
    env = oracle.default_env()
    r = oracle.trim(lattice_trim_params(fb, 1, seed=1).pack(1), fb.TrimState(1), env)
    x = np.repeat(r["x"], N, axis=1)
    x[21:27] = 0; x[12:16] = np.array([1.0, 0, 0, 0])[:, None]            # level, at rest
    y0 = oracle.f_ode(x[:, :1], r["u"], r["ui"], r["s"], env)[1][:, 0]
    x[20] += 1.85 - y0[K["FB_Y_KIN"] + 21]                                  # wheels just compressed on the runway (terrain at 0 m)
    v_r = rng.uniform(16.0, 24.0, N)
    f = (v_r - 16.0) / 8.0
    u = np.repeat(r["u"], N, axis=1)
    u[K["FB_U_THROTTLE"]] = 0.0; u[K["FB_U_FLAPS"]] = 0.3; u[K["FB_U_ELEVATOR"]] = 0.0; u[K["FB_U_AILERON"]] = 0.0; u[K["FB_U_RUDDER"]] = 0.0
    u[K["FB_U_BRAKE_LEFT"]] = 1.0; u[K["FB_U_BRAKE_RIGHT"]] = 1.0          # (the table's `always` actions release them behind the first step)
    u[K["FB_U_M_PILOT"]:K["FB_U_M_PILOT"] + 5] = 0.0
    u[K["FB_U_M_PILOT"]] = 50.0 + 40.0 * f
    ui = np.repeat(r["ui"], N); s = np.repeat(r["s"], N, axis=1)
    par = np.stack([v_r, 0.6 - 0.2 * f])
    scn = ground_table()
    blob = scn.pack(model="Cessna172Sv0")
    order = np.argsort(v_r)

    def check(label, phase, T, status):
        print(f"{label}: lift-off {np.nanmin(T):.2f}..{np.nanmax(T):.2f} s ({np.unique(T).size} distinct steps), phases {np.bincount(phase, minlength=3)}, terminated {int((status != 0).sum())}")
        assert (status == 0).all() and (phase == 2).all() and np.isfinite(T).all(), label
        assert (np.diff(T[order]) >= 0).all(), label + ": lift-off must come in the order of v_r"
        assert np.unique(T).size > 20

    # the oracle, one step at a time, with the table on its arrays
    xo, so, uo, uio = x.copy(), s.copy(), u.copy(), ui.copy()
    st = table_state(N, scn, par)
    status = np.zeros(N, np.int32)
    for k in range(1, steps + 1):
        xo, so, stt = oracle.step(xo, uo, uio, so, env, DT, 1, threads=16)
        status |= stt
        st.update(step=k, u=uo, ui=uio, s=so, active=status == 0, **outputs_for_table(K, oracle.f_ode(xo, uo, uio, so, env)[1]))
        sc.evaluate_on_host(blob, st, k * DT, DT)
    check("oracle", st["phase"], st["rec"][0], status)
    runs = []
    for mode in ("callback", "device"):
        w = fb.BatchedWorld(N)
        w.set_state(x, s); w.u = u; w.ui = ui
        runs.append(run_callback(fb, w, scn, par, steps, reads_y=True) if mode == "callback" else run_table_on_device(fb, w, scn, par, steps, DT))
        w.close()
    a, b = runs
    check("device", b["phase"], b["rec"][0], b["status"])
    assert_same_run(a, b, "ground")
    dT = np.abs(b["rec"][0] - st["rec"][0])
    print(f"device against the oracle's phase machine: lift-off differs by at most {dT.max() / DT:.0f} steps")


# ---- 5. against the oracle's phase machine ----------------------------------------------------------------------------------------------
def test_pitch_table_against_the_oracles_phase_machine(fb, oracle):
    """256 aircraft, case 3's table: on the device, and on the CPU oracle stepped one step at a time with evaluate_on_host on ITS outputs behind each
    step. Both start from the oracle's trim and the thresholds are formed from the oracle's trimmed θ, so every number the comparison depends on is
    made on the CPU. Entry steps and phases must be IDENTICAL, which is a fair demand because every rule that fired on the oracle was clear of its
    threshold by more than 1e-6 x scale (scale 1: an angle, a climb rate around zero, a time) at the step before and at the step of firing — asserted
    here for all 256 — and the state agrees to the project's 1e-6 (support.state_scale)."""
    from flightbatch import scenario as sc
    K = fb.K
    n = 256
    rng = np.random.default_rng(12)
    env = oracle.default_env()
    r = oracle.trim(pitch_trim(fb, rng, n).pack(n), fb.TrimState(n), env, threads=16)
    assert r["ok"].all()
    theta0 = oracle.f_ode(r["x"], r["u"], r["ui"], r["s"], env)[1][K["FB_Y_KIN"] + 1]
    par = pitch_params(rng, theta0, n)
    scn = pitch_table()
    blob = scn.pack(model="Cessna172Sv0")
    xo, so, uo, uio = r["x"].copy(), r["s"].copy(), r["u"].copy(), r["ui"].copy()
    st = table_state(n, scn, par)
    status = np.zeros(n, np.int32)
    lhs_prev = None
    margin = np.full((3, n), np.inf)     # per rule (= per phase left): the smaller of |lhs - threshold| at the step before and at the step of firing
    for k in range(1, PITCH_STEPS + 1):
        xo, so, stt = oracle.step(xo, uo, uio, so, env, DT, 1, threads=16)
        status |= stt
        out = outputs_for_table(K, oracle.f_ode(xo, uo, uio, so, env)[1])
        lhs = np.stack([k * DT - par[3], out["theta"] - par[1], out["clm"]])      # the three rules' left-hand sides minus their thresholds (0)
        before = st["phase"].copy()
        st.update(step=k, u=uo, ui=uio, s=so, active=status == 0, **out)
        sc.evaluate_on_host(blob, st, k * DT, DT)
        fired = np.flatnonzero(st["phase"] != before)
        for i in fired:
            p = before[i]
            margin[p, i] = min(abs(lhs[p, i]), abs(lhs_prev[p, i]) if lhs_prev is not None else np.inf)
        lhs_prev = lhs
    assert (status == 0).all() and (st["phase"] == 3).all(), np.bincount(st["phase"], minlength=4)
    print("oracle: smallest distance of a firing rule from its threshold (step before / step of firing): clock %.3g s, θ %.3g rad, climb rate %.3g m/s"
          % tuple(margin.min(1)))
    assert (margin > 1e-6).all(), np.argwhere(margin <= 1e-6)
    w = fb.BatchedWorld(n)
    w.set_state(r["x"], r["s"]); w.u = r["u"]; w.ui = r["ui"]
    b = run_table_on_device(fb, w, scn, par, PITCH_STEPS, DT)
    w.close()
    err = np.abs(b["x"] - xo) / state_scale(xo, "WA")
    print("device table against the oracle's phase machine, %d steps: max scaled state error %.2e" % (PITCH_STEPS, err.max()))
    assert (b["status"] == 0).all()
    assert np.array_equal(b["phase"], st["phase"]) and np.array_equal(b["since"], st["since"])
    assert _same(b["rec"][0], st["rec"][0])     # (the recorded time is the step of firing x dt)
    assert np.abs(b["rec"][1] - st["rec"][1]).max() < 1e-6 and (np.abs(b["rec"][2] - st["rec"][2]) / np.maximum(st["rec"][2], 1.0)).max() < 1e-6
    assert np.array_equal(b["u"], uo)
    assert err.max() < 1e-6


# ---- 6. the launch partition is invisible -------------------------------------------------------------------------------------------------
def test_launch_partition_is_invisible(fb):
    """steps_per_launch 1, 7 and 50 under a table evaluated after every step, and under one evaluated every 4th step (where the launches really are
    1, 4 and 4 steps long, cut at the evaluation instants): identical bits."""
    ref = pitch_device_run(fb, "WA", spl=50)
    for spl in (1, 7):
        assert_same_run(ref, pitch_device_run(fb, "WA", spl=spl), f"every step, {spl} steps per launch")
    ref4 = pitch_device_run(fb, "WA", spl=50, every=4)
    assert (ref4["phase"] == 3).all() and (ref4["since"] % 4 == 0).all() and not _same(ref4["since"], ref["since"])
    for spl in (1, 7):
        assert_same_run(ref4, pitch_device_run(fb, "WA", spl=spl, every=4), f"every 4th step, {spl} steps per launch")


# ---- 7. environment rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kin", KINS)
def test_table_on_a_handle_with_environment_rows(fb, kin):
    """fb_set_env rows that repeat the batch-wide block: env_any(a, i) reads the aircraft's rows in the table's evaluation (and the PERENV instances
    of the stepping kernels fly it): same arithmetic, to rounding. Same phases and entry steps; the state within the bounds
    test_crosswind_landing_wind_dispersion sets for this kind of comparison (times 0.05 s, positions 1 m) and within the project's airborne
    1e-6, scaled, which is the tighter of the two here."""
    a = pitch_device_run(fb, kin)
    b = pitch_device_run(fb, kin, env_rows=True)
    assert np.array_equal(a["phase"], b["phase"]) and np.array_equal(a["since"], b["since"]) and (b["status"] == 0).all()
    assert np.abs(a["rec"][0] - b["rec"][0]).max() < 0.05
    sc_ = np.maximum(np.abs(a["x"]), 1.0) if kin != "WA" else state_scale(a["x"])
    err = np.abs(a["x"] - b["x"]) / sc_
    d_rec = np.abs(a["rec"] - b["rec"]).max(1)
    print(f"{kin}: rows = the batch-wide block: max scaled state difference {err.max():.2e}; records differ by {d_rec[0]:.1e} s, {d_rec[1]:.1e} rad, {d_rec[2]:.1e} m/s")
    assert err.max() < 1e-6 and np.abs(a["x"] - b["x"]).max() < 1.0
    assert d_rec[1] < 1e-6 and d_rec[2] < 1e-6 * np.maximum(a["rec"][2], 1.0).min()


# ---- 8. checkpoint ---------------------------------------------------------------------------------------------------------------------------
def test_scenario_state_of_a_cessna172sv0_survives_a_checkpoint(fb):
    """Interrupted at step 40 (aircraft in the first three phases: the clock rule fires at steps 6..50, the θ rule from step 28 on) -> checkpoint -> np.savez -> a fresh BatchedWorld -> restore -> the remaining steps:
    bit for bit the uninterrupted run (table, period, parameters, phase, entry step and records travel with the checkpoint)."""
    ref = pitch_device_run(fb, "WA")
    rng = np.random.default_rng(12)
    tp = pitch_trim(fb, rng, N)
    w = fb.BatchedWorld(N)
    fb.f_init(w, tp)
    sim = fb.Simulation(w, dt=DT, save_on=False, steps_per_launch=50)
    w.set_scenario(pitch_table(), params=ref["par"], every=1, rec_init=np.nan)
    fb.step(sim, 40 * DT); w.sync()
    mid = w.scenario_state()["phase"]
    assert np.unique(mid).size >= 3, np.bincount(mid)
    buf = io.BytesIO(); np.savez(buf, **fb.checkpoint(sim)); buf.seek(0)
    w.close()
    ck = dict(np.load(buf))
    w2 = fb.BatchedWorld(N)
    sim2 = fb.Simulation(w2, dt=DT, save_on=False, steps_per_launch=50)
    fb.restore(sim2, ck)
    fb.step(sim2, (PITCH_STEPS - 40) * DT); w2.sync()
    assert_same_run(ref, scenario_result(w2), "resumed")
    w2.close()


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------------------
def test_elevator_step_example_device_table_equals_host_callback(fb):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import elevator_step as demo
    a = demo.run(n=64, seed=2)
    b = demo.run(n=64, seed=2, mode="device")
    assert (a["status"] == 0).all() and (b["status"] == 0).all() and (b["phase"] == 1).all()
    for k in ("x", "s", "u", "ui", "theta", "q"):
        assert _same(a[k], b[k]), k
    assert (b["theta"][-1] != b["theta"][0]).all(), "the step must have been applied"
    print("θ nonlinear - linear at the end of the run: %.4f rad at most (printed, not asserted)" % np.abs(b["theta"][-1] - b["theta_lin"][-1]).max())
