"""Scenario tables that reach the world (FB_SCN_SRC_ENV, FB_SCN_DST_ENV, FB_SCN_SRC_Y; csrc/scenario_kernels.hpp, scn_load / fb_step in
csrc/fb_capi.hip): a script sets the aircraft's own wind rows and reads any row of mdl.y.

N = 320 aircraft: one full 256-lane group of k_scenario and one partial one; every aircraft switches at its own time (a parameter row), so every
wave holds lanes in different phases. At most 400 steps at dt = 0.02. The host side of every bit-for-bit comparison is the SAME table run by
flightbatch.scenario.host_callback (evaluate_on_host behind every step of a Simulation(user_callback=...))."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

from support import (assert_same_run, load_scenario_blob as _load, run_table_as_callback, run_table_on_device, same as _same, scenario_result, state_scale,
                     table_state)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DT = 320, 0.02
GUST_STEPS = 200


def _err(fb):
    return fb.lib.fb_last_error()


# ---- the gust table ------------------------------------------------------------------------------------------------------------------------
def gust_table():
    """At the aircraft's own time (parameter row 0) the east wind steps to row 1 and the north wind by row 2, the down wind is read back into a
    record and T recorded; afterwards the east wind is assigned again at every evaluation (what is there already: no write)."""
    from flightbatch import scenario as sc
    scn = sc.Scenario(n_par=3, n_rec=2)
    CALM, GUST = scn.phase("calm"), scn.phase("gust")
    scn.when(CALM, sc.src.T - sc.par(0) >= 0.0, [sc.env("WIND_E", sc.par(1)), sc.env("WIND_N", sc.env_("WIND_N") + sc.par(2)), sc.rec(0, sc.src.T),
                                                 sc.rec(1, sc.env_("WIND_E") - sc.env_("WIND_D"))], then=GUST)
    scn.always(GUST, [sc.env("WIND_E", sc.par(1))])
    return scn


def gust_case(fb, seed=5):
    """trim parameters, environment rows and table parameters (switch times at odd multiples of dt / 2, steps 5 .. 150: never on the threshold)"""
    K = fb.K
    rng = np.random.default_rng(seed)
    tp = fb.TrimParameters(EAS=rng.uniform(38.0, 50.0, N), h_e=rng.uniform(500.0, 2500.0, N), ψ_nb=rng.uniform(-3.0, 3.0, N))
    env = np.zeros((K["FB_NENV"], N))
    env[K["FB_ENV_WIND_N"]] = rng.uniform(-4.0, 4.0, N); env[K["FB_ENV_WIND_E"]] = rng.uniform(-4.0, 4.0, N); env[K["FB_ENV_WIND_D"]] = rng.uniform(-1.0, 1.0, N)
    env[K["FB_ENV_T_SL"]] = rng.uniform(278.0, 298.0, N); env[K["FB_ENV_P_SL"]] = rng.uniform(99000.0, 103000.0, N)
    par = np.stack([(rng.integers(5, 150, N) + 0.5) * DT, rng.uniform(-8.0, 8.0, N), rng.uniform(-3.0, 3.0, N)])
    return tp, env, par


def make_world(fb, model, kin, tp, env):
    w = fb.Cessna172Xv2World(N, kinematics=kin) if model == "x2" else fb.BatchedWorld(N, kinematics=kin)
    w.env = env
    fb.f_init(w, tp)
    assert w.trim_success.all()
    return w


_GUST = {}


def gust_device_run(fb, model="s0", kin="WA", spl=1, every=1):
    key = (model, kin, spl, every)
    if key not in _GUST:
        tp, env, par = gust_case(fb)
        w = make_world(fb, model, kin, tp, env)
        _GUST[key] = run_table_on_device(fb, w, gust_table(), par, GUST_STEPS, DT, spl, every, ratio=2 if model == "x2" else 1)
        _GUST[key]["env0"] = env
        w.close()
    return _GUST[key]


# ---- 1. table = host callback, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kin", [("s0", "WA"), ("s0", "ECEF"), ("s0", "NED"), ("x2", "WA")])
@pytest.mark.parametrize("spl,every", [(1, 1), (50, 25)])
def test_wind_table_equals_the_host_callback(fb, model, kin, spl, every):
    """x, s, u, ui, env, phase, entry step, records and status (Cessna172Xv2: cu, cs too; Δt = 2 dt, so half of the steps have no control update).
    The host side pushes a changed wind through fb_set_env, which drops the carried derivative of every aircraft; the device drops it for the aircraft
    whose wind changed — without that, the Cessna172Xv2 runs differ."""
    K = fb.K
    tp, env, par = gust_case(fb)
    b = gust_device_run(fb, model, kin, spl, every)
    w = make_world(fb, model, kin, tp, env)
    a = run_table_as_callback(fb, w, gust_table(), par, GUST_STEPS, DT, every, ratio=2 if model == "x2" else 1)
    w.close()
    fired = np.ceil(par[0] / DT / every) * every
    print(f"{model} {kin} spl {spl} every {every}: switch at steps {b['since'].min()}..{b['since'].max()} ({np.unique(b['since']).size} distinct)")
    assert (b["status"] == 0).all() and (b["phase"] == 1).all()
    assert np.array_equal(b["since"], fired.astype(np.int64)) and _same(b["rec"][0], fired * DT)
    assert np.unique(b["since"]).size >= (5 if every > 1 else 20)
    WN, WE, WD = K["FB_ENV_WIND_N"], K["FB_ENV_WIND_E"], K["FB_ENV_WIND_D"]
    assert _same(b["env"][WE], par[1]) and _same(b["env"][WN], env[WN] + par[2]) and _same(b["env"][WD:], env[WD:])
    assert _same(b["rec"][1], par[1] - env[WD])          # (WIND_E read after the action before it wrote the row)
    b = {k: v for k, v in b.items() if k != "env0"}
    assert_same_run(a, b, (model, kin, spl, every))


def test_tapped_airspeed_behind_an_always_wind_write(fb):
    """A tailwind that grows with the clock, written by an `always` action at every evaluation, and a rule on the tapped EAS: on the device the walk's
    evaluation of f_ode! stands behind that write (stage A, then B), so the rule sees the new wind; the host callback renews its taps under the new rows.
    The firing rule records the tapped EAS and the record's EAS row (y_: the refresh ahead of the evaluation, under the OLD wind): the two differ.
    Thresholds 0.5 .. 4 m/s below the trimmed EAS, the wind gaining 3 m/s per second on an aircraft heading east: every rule fires within 300 steps."""
    from flightbatch import scenario as sc
    K = fb.K
    steps = 300
    scn = sc.Scenario(n_par=2, n_rec=3)
    RAMP, DONE = scn.phase("ramp"), scn.phase("done")
    scn.always(RAMP, [sc.env("WIND_E", sc.par(0) + 3.0 * sc.src.T)])
    scn.when(RAMP, sc.src.EAS - sc.par(1) < 0.0, [sc.rec(0, sc.src.EAS), sc.rec(1, sc.y_(K["FB_Y_AIR"] + 20)), sc.rec(2, sc.src.T)], then=DONE)
    rng = np.random.default_rng(33)
    EAS = rng.uniform(40.0, 50.0, N)
    tp = fb.TrimParameters(EAS=EAS, h_e=rng.uniform(500.0, 2000.0, N), ψ_nb=np.full(N, np.pi / 2))
    env = np.zeros((K["FB_NENV"], N)); env[K["FB_ENV_T_SL"]] = 288.15; env[K["FB_ENV_P_SL"]] = 101325.0
    par = np.stack([np.zeros(N), EAS - rng.uniform(0.5, 4.0, N)])
    runs = []
    for mode in ("device", "callback"):
        w = make_world(fb, "s0", "WA", tp, env)
        runs.append(run_table_on_device(fb, w, scn, par, steps, DT, spl=50, every=1) if mode == "device" else run_table_as_callback(fb, w, scn, par, steps, DT, every=1))
        w.close()
    b, a = runs
    print(f"EAS rule fired at steps {np.nanmin(b['rec'][2]) / DT:.0f}..{np.nanmax(b['rec'][2]) / DT:.0f}; tapped EAS below the record's by "
          f"{np.nanmin(b['rec'][1] - b['rec'][0]):.4f}..{np.nanmax(b['rec'][1] - b['rec'][0]):.4f} m/s")
    assert (b["status"] == 0).all() and (b["phase"] == 1).all() and np.unique(b["since"]).size > 20
    assert (b["rec"][0] < par[1]).all() and (b["rec"][0] < b["rec"][1]).all()      # one more step of tailwind in the tap than in the record
    assert_same_run(a, b, "tapped EAS behind an always wind write")


# ---- 2. against the oracle ------------------------------------------------------------------------------------------------------------------
def test_wind_table_against_the_oracle_stepped_under_per_aircraft_environments(fb, oracle):
    """Cessna172Sv0, WA, 300 steps: the oracle is stepped one step at a time, each aircraft in its own environment, and the numpy interpreter applies
    the table to those environment rows between the steps. Both start from the oracle's trim. Scaled state error <= 1e-6 (the project's airborne
    bound, support.state_scale); phases, entry steps and wind rows identical (the rules read the clock only)."""
    from flightbatch import scenario as sc
    steps = 300
    tp, env6, par = gust_case(fb, seed=9)
    scn = gust_table()
    blob = scn.pack(model="Cessna172Sv0")
    env_o = env6.copy()
    with oracle.per_aircraft_env():
        r = oracle.trim(tp.pack(N), fb.TrimState(N), oracle.env_rows(env_o), threads=16)
        assert r["ok"].all()
        xo, so, uo, uio = r["x"].copy(), r["s"].copy(), r["u"].copy(), r["ui"].copy()
        st = dict(table_state(N, scn, par), env=env_o)
        status = np.zeros(N, np.int32)
        for k in range(1, steps + 1):
            xo, so, stt = oracle.step(xo, uo, uio, so, oracle.env_rows(env_o), DT, 1, threads=16)
            status |= stt
            st.update(step=k, u=uo, ui=uio, s=so, active=status == 0)
            sc.evaluate_on_host(blob, st, k * DT, DT)
    assert (status == 0).all() and (st["phase"] == 1).all()
    w = fb.BatchedWorld(N)
    w.env = env6
    w.set_state(r["x"], r["s"]); w.u = r["u"]; w.ui = r["ui"]
    b = run_table_on_device(fb, w, scn, par, steps, DT, spl=50, every=1)
    w.close()
    err = np.abs(b["x"] - xo) / state_scale(xo, "WA")
    print("wind table against the oracle, %d steps: max scaled state error %.2e" % (steps, err.max()))
    assert (b["status"] == 0).all()
    assert np.array_equal(b["phase"], st["phase"]) and np.array_equal(b["since"], st["since"]) and _same(b["rec"], st["rec"])
    assert _same(b["env"], env_o) and not _same(env_o, env6)
    assert err.max() <= 1e-6


# ---- 3. FB_SCN_SRC_Y ---------------------------------------------------------------------------------------------------------------------------
def y_table(K):
    """a rule on a row of the airflow block (TAS below the aircraft's threshold), then one on a row of the power-plant block (engine speed below the
    aircraft's threshold); the firing rule copies its row into a record, and the time"""
    from flightbatch import scenario as sc
    TAS, OMEGA = K["FB_Y_AIR"] + 19, K["FB_Y_PWP"] + 3
    scn = sc.Scenario(n_par=2, n_rec=4)
    A, B, C_ = scn.phase("fast"), scn.phase("slowing"), scn.phase("done")
    scn.when(A, sc.y_(OMEGA) - sc.par(1) < 0.0, [sc.rec(1, sc.y_(OMEGA)), sc.rec(3, sc.src.T)], then=B)
    scn.when(B, sc.y_(TAS) - sc.par(0) < 0.0, [sc.rec(0, sc.y_(TAS)), sc.rec(2, sc.src.T)], then=C_)
    return scn, TAS, OMEGA


def y_case(fb):
    """trimmed, then throttle closed and the nose pulled up: engine speed and airspeed fall; thresholds a little below each aircraft's trimmed values"""
    K = fb.K
    rng = np.random.default_rng(21)
    tp = fb.TrimParameters(EAS=rng.uniform(40.0, 50.0, N), h_e=rng.uniform(500.0, 2000.0, N))
    w = fb.BatchedWorld(N)
    fb.f_init(w, tp)
    assert w.trim_success.all()
    u = w.u
    u[K["FB_U_THROTTLE"]] = 0.05; u[K["FB_U_ELEVATOR"]] += 0.06
    w.u = u
    fb.f_ode(w)
    y = w.y
    par = np.stack([y[K["FB_Y_AIR"] + 19] - rng.uniform(1.0, 4.0, N), y[K["FB_Y_PWP"] + 3] * (1.0 - rng.uniform(0.05, 0.30, N))])
    return w, par


def _launches(fb, w, sim, steps):
    fb.lib.fb_timing_begin(w._h)
    fb.step(sim, steps * DT)
    ms, nl = C.c_float(), C.c_int64()
    assert fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)) == 0
    return int(nl.value)


def test_any_output_row_as_a_source(fb):
    K = fb.K
    steps = 400
    scn, TAS, OMEGA = y_table(K)
    w, par = y_case(fb)
    x0, s0, u0, ui0 = w.x, w.s, w.u, w.ui
    b = run_table_on_device(fb, w, scn, par, steps, DT, spl=50, every=1)
    w.close()
    t_tas, t_om = b["rec"][2], b["rec"][3]
    print(f"engine-speed rule fired at steps {np.nanmin(t_om) / DT:.0f}..{np.nanmax(t_om) / DT:.0f}, TAS rule at {np.nanmin(t_tas) / DT:.0f}..{np.nanmax(t_tas) / DT:.0f}; "
          f"phases {np.bincount(b['phase'], minlength=3)}")
    assert (b["status"] == 0).all() and (b["phase"] == 2).all() and np.isfinite(b["rec"]).all()
    assert (b["rec"][0] < par[0]).all() and (b["rec"][1] < par[1]).all()
    k_tas, k_om = np.rint(t_tas / DT).astype(int), np.rint(t_om / DT).astype(int)
    assert np.unique(k_tas).size > 20 and np.unique(k_om).size > 5
    # a second run without the table (it writes records only), stopped at every firing step: fb_f_ode + fb_get_output_fields there
    w2 = fb.BatchedWorld(N)
    w2.set_state(x0, s0); w2.u = u0; w2.ui = ui0
    sim2 = fb.Simulation(w2, dt=DT, save_on=False, steps_per_launch=50)
    done = 0
    for k in sorted(set(k_tas) | set(k_om)):
        fb.step(sim2, (k - done) * DT); done = k
        fb.f_ode(w2)
        air, pwp = w2.y_fields("AIR"), w2.y_fields("PWP")
        m = k_tas == k
        assert _same(b["rec"][0][m], air[19][m]), k
        m = k_om == k
        assert _same(b["rec"][1][m], pwp[3][m]), k
    w2.close()


def test_a_table_without_output_rows_pays_no_refresh(fb):
    """fb_timing_end's launch count: 100 steps under a table evaluated behind every step are 100 stepping launches — and 100 refreshes of the output
    record on top only for the table that names FB_SCN_SRC_Y"""
    K = fb.K
    tp, env, par = gust_case(fb)
    w = make_world(fb, "s0", "WA", tp, env)
    sim = fb.Simulation(w, dt=DT, save_on=False, steps_per_launch=50)
    assert _launches(fb, w, sim, 100) == 2
    w.set_scenario(gust_table(), params=par, every=1)
    assert _launches(fb, w, sim, 100) == 100
    w.set_scenario(gust_table(), params=par, every=25)
    assert _launches(fb, w, sim, 100) == 4
    scn, _, _ = y_table(K)
    w.set_scenario(scn, params=np.zeros((2, N)), every=1)
    assert _launches(fb, w, sim, 100) == 200
    w.set_scenario(scn, params=np.zeros((2, N)), every=25)
    assert _launches(fb, w, sim, 100) == 8
    w.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(fb):
    from flightbatch import scenario as sc
    K = fb.K
    n = 64

    def raw(action=None, cond=None):
        """a packed one-rule table; rows pack() would refuse are patched into the blob afterwards"""
        scn = sc.Scenario(n_par=1, n_rec=1)
        a, b = scn.phase("a"), scn.phase("b")
        scn.when(a, cond if cond is not None else sc.src.T >= 1.0, [action] if action is not None else [], then=b)
        return scn.pack()

    rule0 = K["FB_SCN_HDR"] + 2 * K["FB_SCN_PHASE_REC"]
    act0 = rule0 + K["FB_SCN_RULE_REC"]
    good = raw(sc.rec(0, sc.src.T))
    wind = raw(sc.env("WIND_E", sc.par(0)))
    reads = raw(sc.rec(0, sc.env_("P_SL")))
    cond = raw(cond=sc.env_("H_TERRAIN") > 0.0)

    def dst_row(row):
        b = wind.copy(); b[act0 + 1] = row
        return b

    for kin in ("WA", "ECEF", "NED"):
        w = fb.BatchedWorld(n, kinematics=kin)
        # ENV kinds on a handle without rows
        for blob in (wind, reads, cond):
            assert _load(fb, w, blob) != 0 and b"fb_set_env" in _err(fb), _err(fb)
            assert fb.lib.fb_scenario_configure(w._h, 1) != 0 and b"no scenario table" in _err(fb)
        with pytest.raises(fb.FlightBatchError, match="fb_set_env"):
            w.set_scenario(_scn_with(sc, sc.env("WIND_N", 1.0)))
        assert _load(fb, w, good) == 0
        w.set_env()
        for blob in (wind, reads, cond):
            assert _load(fb, w, blob) == 0
        # destinations other than the wind
        for row, why in ((K["FB_ENV_T_SL"], b"derived rows"), (K["FB_ENV_P_SL"], b"derived rows"), (K["FB_ENV_H_TERRAIN"], b"constructor argument")):
            assert _load(fb, w, dst_row(row)) != 0 and why in _err(fb) and b"FB_ENV_WIND_N" in _err(fb), (row, _err(fb))
            assert _load(fb, w, good) == 0
        assert _load(fb, w, dst_row(K["FB_NENV"])) != 0 and b"destination row" in _err(fb)
        # source rows
        b_ = reads.copy(); b_[act0 + 6] = K["FB_NENV"]
        assert _load(fb, w, b_) != 0 and b"source row" in _err(fb)
        yb = raw(sc.rec(0, sc.y_(K["FB_NY"] - 1)))
        assert _load(fb, w, yb) == 0
        yb[act0 + 6] = K["FB_NY"]
        assert _load(fb, w, yb) != 0 and b"source row" in _err(fb)
        yc = raw(cond=sc.y_(3) > 0.0); yc[rule0 + 1] = K["FB_NY"]
        assert _load(fb, w, yc) != 0 and b"source row" in _err(fb)
        assert _load(fb, w, good) == 0
        # the rows must stay while a table names them
        assert _load(fb, w, wind) == 0
        assert fb.lib.fb_set_env(w._h, None) != 0 and b"fb_scenario_configure" in _err(fb)
        with pytest.raises(fb.FlightBatchError, match="fb_scenario_configure"):
            w.env = None
        assert w.has_env
        w.set_scenario(None)
        w.env = None
        assert not w.has_env
        w.set_env()
        assert _load(fb, w, good) == 0 and fb.lib.fb_set_env(w._h, None) == 0      # (a table that names no environment row does not hold them)
        w.close()
    for blob in (wind, raw(sc.rec(0, sc.y_(3)))):
        f32 = fb.BatchedWorld(n, dtype="f32")
        f32.set_env()
        assert _load(fb, f32, blob) != 0 and b"FB_F32" in _err(fb)
        f32.close()
        r2 = fb.Robot2DWorld(n)
        assert _load(fb, r2, blob) != 0 and b"another model family" in _err(fb)
        r2.close()


def _scn_with(sc, action):
    scn = sc.Scenario(n_par=0, n_rec=0)
    scn.always(scn.phase("a"), [action])
    return scn


# ---- 5. status -------------------------------------------------------------------------------------------------------------------------------------
def test_terminated_aircraft_keep_their_wind(fb):
    K = fb.K
    tp, env, par = gust_case(fb)
    par[0] = 10.5 * DT
    w = make_world(fb, "s0", "WA", tp, env)
    status = np.zeros(N, np.int32)
    dead = np.array([0, 7, 63, 64, 100, 255, 256, 319])
    status[dead] = K["FB_ST_ALT_RANGE"]
    assert fb.lib.fb_set_status(w._h, status.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    b = run_table_on_device(fb, w, gust_table(), par, 30, DT, spl=50, every=1)
    w.close()
    alive = status == 0
    assert np.array_equal(b["status"], status)
    assert _same(b["env"][:, dead], env[:, dead]) and (b["phase"][dead] == 0).all() and np.isnan(b["rec"][:, dead]).all()
    assert _same(b["env"][K["FB_ENV_WIND_E"], alive], par[1, alive]) and (b["phase"][alive] == 1).all() and (b["since"][alive] == 11).all()


# ---- 6. checkpoint ---------------------------------------------------------------------------------------------------------------------------------
def test_wind_table_survives_a_checkpoint(fb):
    """Interrupted at step 80 (the aircraft switch at steps 6 .. 150) -> checkpoint (state, inputs, environment rows, scenario state) -> np.savez -> a
    fresh BatchedWorld -> restore -> the remaining steps: bit for bit the uninterrupted run."""
    ref = gust_device_run(fb, "s0", "WA", 50, 1)
    tp, env, par = gust_case(fb)
    w = make_world(fb, "s0", "WA", tp, env)
    sim = fb.Simulation(w, dt=DT, save_on=False, steps_per_launch=50)
    w.set_scenario(gust_table(), params=par, every=1, rec_init=np.nan)
    fb.step(sim, 80 * DT); w.sync()
    mid = w.scenario_state()["phase"]
    assert 0 < mid.sum() < N and not _same(w.env, env)
    buf = io.BytesIO(); np.savez(buf, **fb.checkpoint(sim)); buf.seek(0)
    w.close()
    ck = dict(np.load(buf))
    w2 = fb.BatchedWorld(N)
    sim2 = fb.Simulation(w2, dt=DT, save_on=False, steps_per_launch=50)
    fb.restore(sim2, ck)
    fb.step(sim2, (GUST_STEPS - 80) * DT); w2.sync()
    assert_same_run({k: v for k, v in ref.items() if k != "env0"}, scenario_result(w2), "resumed")
    w2.close()


# ---- 7. the example -------------------------------------------------------------------------------------------------------------------------------
def test_wind_shear_landing_example(fb):
    """64 aircraft from 1.1 - 1.5 km out (the run is 70 s instead of the demo's 150: what is asserted happens before the roll-out ends): device table =
    host callback bit for bit; every aircraft on the ground, none terminated; the lateral offset at touchdown grows with the size of the shear over
    three bins. The offset is measured from where the aircraft that meet NO shear touch down (every fourth aircraft, interleaved over the lanes): under
    track hold the crosswind of the final leg leaves a cross-track bias of its own, the same for all, and what the shear does is the displacement from it."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import wind_shear_landing as demo
    n = 64
    group = np.arange(n) % 4                                                              # 0: no shear; 1, 2, 3: 0-2, 2-4, 4-6 m/s
    shear = np.where(group == 0, 0.0, (group - 1) * 2.0 + np.random.default_rng(4).uniform(0.0, 2.0, n))
    kw = dict(n=n, t_end=70.0, s0_range=(1100.0, 1500.0), seed=3, shear=shear, crosswind=np.full(n, 3.0), shear_height=np.full(n, 15.0))
    b = demo.run(mode="device", **kw)
    a = demo.run(mode="callback", **kw)
    for k in ("x", "s", "u", "ui", "cu", "cs", "env", "status", "phase", "since", "rec"):
        assert _same(np.asarray(a[k]), np.asarray(b[k])), k
    assert (b["status"] == 0).all() and (b["phase"] == 4).all() and np.isfinite(b["rec"]).all()
    assert _same(b["env"][fb.K["FB_ENV_WIND_E"]], 3.0 + shear)
    e = [b["rec"][2][group == j].mean() for j in range(4)]
    d = [abs(e[j] - e[0]) for j in (1, 2, 3)]
    print("mean cross-track at touchdown: no shear %+.3f m; shear 0-2, 2-4, 4-6 m/s: %+.3f %+.3f %+.3f m; displaced by %.3f %.3f %.3f m" % (*e, *d))
    assert 0.0 < d[0] < d[1] < d[2]
