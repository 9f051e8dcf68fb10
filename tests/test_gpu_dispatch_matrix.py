"""Every stepping-kernel instance that launch_step (csrc/fb_capi.hip) can select, against the CPU oracle, on one batch that gives the
instance real work: airborne lanes, lanes that change pass through the 10 m band, and lanes in ground contact, in every wave.

launch_step names the kernel from four run-time properties of the handle (model, mechanisation, per-aircraft environment rows,
FLIGHTBATCH_DUO). A wrong template argument there compiles, and flies the aircraft in the wrong environment or hands a lane to the wrong
ground-capable instance; this file is where the mapping from handle to instance is checked.

    case (test id)                      airborne pass                            ground-capable pass behind it
    ----------------------------------  ---------------------------------------  ------------------------------------------
    {Sv0|Xv2}-{WA|ECEF|NED}-block-duo   k_step_duo<KIN, X, false>                k_step_air<KIN, X, true, false>
    {Sv0|Xv2}-{WA|ECEF|NED}-rows-duo    k_step_duo<KIN, X, true>                 k_step_air<KIN, X, true, true>
    {Sv0|Xv2}-{WA|ECEF|NED}-block-air   k_step_air<KIN, X, false, false>         k_step_air<KIN, X, true, false>
    {Sv0|Xv2}-{WA|ECEF|NED}-rows-air    k_step_air<KIN, X, false, true>          k_step_air<KIN, X, true, true>
    f32-block                           fbf::k_step_f32                          k_step_air<WA, false, true, false>
    f32-rows                            k_step_air<WA, false, false, true>       k_step_air<WA, false, true, true>
  (KIN: 0 WA, 1 ECEF, 2 NED; X: false Cessna172Sv0, true Cessna172Xv2; "air" = FLIGHTBATCH_DUO=0, read when the handle is created.)
24 + 2 cases: 12 k_step_duo, 12 airborne k_step_air, the one k_step_f32, and each of the 12 ground-capable k_step_air twice — the 37
k_step_* symbols tests/test_kernel_resources.py finds in the code object. AN INSTANCE ADDED TO launch_step GETS A ROW HERE.

The batch (drawn once per model from a fixed seed, N = 768 + 37: a tail block and a partial wave), scattered in latitude, longitude
and heading (ECEF and NED differ from WA only away from ϕ = λ = ψ = 0), every aircraft over ITS OWN terrain elevation plus the geoid
undulation at its position, three groups mixed within every wave:
    1  airborne throughout: lattice trims, perturbed in rates and velocity (Xv2: every aircraft in its own pair of modes);
    2  through the 10 m hand-over band without touching down: Xv2 descends and levels off at 5-8 m (EAS_alt) or climbs out (EAS_clm);
       Sv0, which has no autopilot, flies trimmed shallow descents and climbs;
    3  ground contact: approaches at 2-4° that touch down (Xv2: a part of them under EAS_clm), and aircraft that start on their wheels.
With per-aircraft rows every row (wind, T_sl, p_sl, terrain elevation) differs between neighbours.

The reference is the oracle in the same mechanisation and environment, started from the device's start state and stepped ONE step at a
time, so that band crossings (orthometric clearance: h_e less the geoid undulation at the start position — the aircraft move less than
300 m, the undulation with them by centimetres — less the aircraft's own terrain elevation) and weight on wheels (f_ode! on the lanes
within 4 m of their terrain) are counted on the oracle alone, and asserted: a retune cannot quietly take the work away from an instance.
Tolerances are those of the nearest instance already covered (tests/test_gpu_env.py, test_gpu_parity.py, test_gpu_f32.py).
"""
import contextlib
import os
import sys

import numpy as np
import pytest

from oracle_binding import OracleX
from support import H_E_ROW, N_KIN, abi_to_oracle_rows, digest_dict, geoid, random_env, state_scale, stepper

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import F32_TOLERANCE   # noqa: E402

pytestmark = pytest.mark.gpu

N = 768 + 37                     # neither a multiple of 256 nor of 64
NSTEPS = 500
DT = 0.01
RATIO = 2                        # Cessna172Xv2: Δt = 2 dt
BAND = 10.0                      # the airborne pass's clearance limit (orthometric height over the terrain)
NEAR = 4.0                       # weight on wheels is looked for below this clearance (gear legs ~1.9 m)
H_TRN = 120.0                    # the batch-wide block's terrain elevation
TOL = 1e-6                       # airborne lanes: scaled state / control-law record (test_gpu_env.py, test_gpu_parity.py)
TOL_GROUND = 1e-3                # lanes in ground contact: altitude and attitude (test_per_aircraft_terrain_elevation_ground_contact)
ATT = {"WA": slice(12, 16), "ECEF": slice(12, 16), "NED": slice(12, 15)}   # q_wb / q_eb / (ψ, θ, φ)


_SCENARIO = {}


def scenario(fb, oracle, x2, rows):
    """trim parameters, environment, groups, the perturbation of the start state and the control-law inputs (drawn once per model and
    environment from one seed: the draws are the same whichever mechanisation or stepper flies them)"""
    if (x2, rows) in _SCENARIO:
        return _SCENARIO[(x2, rows)]
    K = fb.K
    rng = np.random.default_rng(2718)

    def U(a, b):
        return rng.uniform(a, b, N)
    grp = rng.integers(1, 4, N)
    sub = rng.random(N)
    g1, g2, g3 = grp == 1, grp == 2, grp == 3
    down, up = g2 & (sub < 0.5), g2 & (sub >= 0.5)
    appr, wheels = g3 & (sub < 0.7), g3 & (sub >= 0.7)
    lat, lon, psi = U(-1.2, 1.2), U(-np.pi, np.pi), U(-np.pi, np.pi)
    h_own = U(20.0, 400.0)
    h_trn = h_own if rows else np.full(N, H_TRN)
    N0 = geoid(oracle, lat, lon)
    # group 1: the lattice of support.lattice_trim_params, over the aircraft's own terrain
    clr1 = U(200.0, 3000.0)          # clearance over the terrain, m
    eas1 = U(35.0, 55.0)
    gam1 = U(-0.02, 0.02)            # flight-path angle, rad
    pdot1 = U(-0.03, 0.03)           # turn rate, rad/s
    flaps1 = rng.choice([0.0, 0.0, 0.33], N)
    fuel = U(0.1, 1.0)
    # group 2, descending (_d) and climbing (_u): start clearance, flight-path angle, airspeed
    if x2:   # (a) and (c) of test_gpu_launch_edges.py
        clr_d = U(12.0, 30.0)
        gam_d = -U(0.03, 0.06)
        clr_u = U(4.0, 9.0)
        gam_u = U(0.02, 0.05)
        eas2 = U(42.0, 55.0)
    else:    # trimmed: at most 0.025 x 50 m/s x 5 s = 6.3 m down from at least 10.3 m
        clr_d = U(10.3, 12.5)
        gam_d = -U(0.015, 0.025)
        clr_u = U(5.0, 9.5)
        gam_u = U(0.02, 0.05)
        eas2 = U(38.0, 50.0)
    # group 3: test_per_aircraft_terrain_elevation_ground_contact's approaches; the rest start on their wheels, rolling
    clr_a = U(4.0, 13.0)
    gam_a = -np.deg2rad(U(2.0, 4.0))
    eas3 = U(33.0, 40.0)
    clr_w = U(1.75, 1.90)            # on the wheels: height of the reference point over the terrain
    vscale = U(0.2, 0.6)             # ... and the share of the trimmed speed they roll at
    # (the aircraft on their wheels are trimmed in free air, 3 m up — a trim with the gear loaded is not one — and then set down)
    clr0 = np.select([g1, down, up, appr], [clr1, clr_d, clr_u, clr_a], 3.0)
    tp = fb.TrimParameters(n_e=np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)]), h_e=h_trn + N0 + clr0, ψ_nb=psi,
                           EAS=np.select([g1, g2], [eas1, eas2], eas3), γ_wb_n=np.select([g1, down, up, appr], [gam1, gam_d, gam_u, gam_a], 0.0),
                           ψ_wb_dot=np.where(g1, pdot1, 0.0), flaps=np.select([g1, g2], [flaps1, 0.0], 1.0), fuel_load=fuel)
    env6 = None
    if rows:
        env6 = random_env(fb, N, 29, h_trn=h_trn)
        env6[K["FB_ENV_WIND_N"]:K["FB_ENV_WIND_D"] + 1] *= np.where(g1, 1.0, 0.3)      # near the ground: a light wind
        assert (np.diff(env6, axis=1) != 0).all(), "every row must differ between neighbours"
    amp = np.select([g1, g2], [1.0, 0.2], 0.0)
    dw = rng.normal(0, 0.02, (3, N)) * amp       # off trim in body rates, rad/s
    dv = rng.normal(0, 1.0, (3, N)) * amp        # ... and in velocity, m/s
    # Cessna172Xv2, group 1: every aircraft in its own pair of modes, references off the trimmed ones
    lon_req = rng.integers(0, 9, N)
    lat_req = rng.integers(0, 5, N)
    d_eas = U(-3, 3)
    d_clm = U(-1.5, 1.5)
    d_phi = U(-0.3, 0.3)
    d_chi = U(-0.5, 0.5)
    # ... groups 2 and 3: climb-rate references, and the height over the terrain at which the descents level off
    clm_d = -U(1.5, 3.5)
    clm_u = U(1.5, 3.0)
    clm_a = -U(1.2, 2.5)
    dh = U(5.0, 8.0)
    auto_a = appr & (sub < 0.35)

    def perturb(x, kin):
        """the start state in C ABI order: groups 1 and 2 off trim in rates and velocity, the aircraft on their wheels set down and slowed to a roll"""
        d0 = (K["FB_X2_KIN"] if x2 else 12) + N_KIN[kin]
        x = x.copy()
        x[d0:d0 + 3] += dw
        x[d0 + 3:d0 + 6] += dv
        x[d0 + 3:d0 + 6, wheels] *= vscale[wheels]
        x[d0 - 1, wheels] -= (3.0 - clr_w)[wheels]       # (h_e is the last kinematic row of every mechanisation)
        return x

    def set_cu(cu):
        ModeLon, ModeLat = fb.ModeControlLon, fb.ModeControlLat
        cu = cu.copy()
        lonm, latm = cu[K["FB_CU_LON_MODE_REQ"]], cu[K["FB_CU_LAT_MODE_REQ"]]
        lonm[g1], latm[g1] = lon_req[g1], lat_req[g1]
        for row, d in (("EAS_REF", d_eas), ("CLM_REF", d_clm), ("PHI_REF", d_phi), ("CHI_REF", d_chi)):
            cu[K["FB_CU_" + row], g1] += d[g1]
        lonm[down] = float(ModeLon.EAS_alt)
        lonm[up | auto_a] = float(ModeLon.EAS_clm)
        latm[g2 | auto_a] = float(ModeLat.φ_β)
        cu[K["FB_CU_CLM_REF"]] = np.select([down, up, auto_a], [clm_d, clm_u, clm_a], cu[K["FB_CU_CLM_REF"]])
        cu[K["FB_CU_H_REF"], down] = (h_trn + N0 + dh)[down]          # (an ellipsoidal altitude)
        cu[K["FB_CU_EAS_REF"], g2 | auto_a] = np.asarray(tp.EAS)[g2 | auto_a]
        return cu
    sc = dict(tp=tp, env6=env6, h_trn=h_trn, N0=N0, groups={1: g1, 2: g2, 3: g3}, perturb=perturb, set_cu=set_cu)
    _SCENARIO[(x2, rows)] = sc
    return sc


@contextlib.contextmanager
def mechanisation(fb, oracle, kin, rows):
    """the oracle in mechanisation `kin`, with one environment per aircraft when `rows`"""
    with oracle.per_aircraft_env() if rows else contextlib.nullcontext():
        oracle.lib.fo_set_kinematics(fb.K["FB_KIN_" + kin])
        try:
            yield
        finally:
            oracle.lib.fo_set_kinematics(fb.K["FB_KIN_WA"])


_TRIM_OK = {}


def oracle_trim_ok(fb, oracle, x2, kin, rows):
    """which aircraft the oracle's own trim of the scenario converges for (is the device's trim the same aircraft?)"""
    if (x2, kin, rows) in _TRIM_OK:
        return _TRIM_OK[(x2, kin, rows)]
    sc = scenario(fb, oracle, x2, rows)
    env = oracle.env_rows(sc["env6"]) if rows else oracle.default_env(h_trn=H_TRN)
    tp = sc["tp"].pack(N)
    with mechanisation(fb, oracle, kin, rows):
        if x2:
            o = OracleX(oracle, fb.ctl_gains.ctl_gains_blob()).trim_init(tp, fb.TrimState(N), env, DT * RATIO, threads=16)
        else:
            o = oracle.trim(tp, fb.TrimState(N), env, threads=16)
    ok = _TRIM_OK[(x2, kin, rows)] = np.asarray(o["ok"]).copy()
    return ok


_ORACLE = {}


def oracle_run(fb, oracle, x2, kin, env, start, h_trn, N0):
    """NSTEPS of the oracle from `start` (arrays in C ABI order), one step at a time: the final state (oracle layout), status and
    termination record, and per aircraft whether its clearance was ever below the band, how often it crossed it, its lowest clearance,
    and the first step with weight on wheels (-1: never)"""
    K = fb.K
    rows = env.ndim == 2
    key = (x2, kin, digest_dict(start), digest_dict(dict(env=env, h=h_trn)))
    if key in _ORACLE:
        return _ORACLE[key]
    rmap = abi_to_oracle_rows(K, "x2" if x2 else "s0", kin)
    x = np.zeros((34 if x2 else 27, N)); x[rmap] = start["x"]
    hrow, ldg = H_E_ROW[kin], K["FB_Y_LDG"]
    X = OracleX(oracle, fb.ctl_gains.ctl_gains_blob()) if x2 else None
    o = dict(x=x, u=start["u"].copy(), ui=start["ui"].copy(), s=start["s"].copy(), status=np.zeros(N, np.int32), nstep=0,
             term_step=np.full(N, -1, np.int64), term_where=np.zeros(N, np.int32))
    if x2:
        o["cu"], o["cs"] = start["cu"].copy(), start["cs"].copy()
    below = np.zeros((NSTEPS + 1, N), bool)
    first_wow = np.full(N, -1)
    min_clr = np.full(N, np.inf)

    def look(k):
        clr = o["x"][hrow] - N0 - h_trn
        below[k] = clr < BAND
        np.minimum(min_clr, clr, out=min_clr)
        idx = np.nonzero((clr < NEAR) & (first_wow < 0) & (o["status"] == 0))[0]
        if len(idx):
            e = np.ascontiguousarray(env[:, idx]) if rows else env
            if x2:
                sub = {k_: np.ascontiguousarray(o[k_][..., idx]) for k_ in ("x", "u", "ui", "s", "cs")}
                y = X.f_ode(sub, e)[1]
            else:
                y = oracle.f_ode(o["x"][:, idx], o["u"][:, idx], o["ui"][idx], o["s"][:, idx], e)[1]
            first_wow[idx[(y[ldg + 1] + y[ldg + 12] + y[ldg + 23]) > 0]] = k
    with mechanisation(fb, oracle, kin, rows):
        look(0)
        for k in range(NSTEPS):
            if x2:
                X.step_term(o, env, DT, RATIO, 1, threads=16)
            else:
                o["x"], o["s"], o["status"], ts, tw = oracle.step_term(o["x"], o["u"], o["ui"], o["s"], env, DT, 1, step0=k, status=o["status"], threads=16)
                new = (ts >= 0) & (o["term_step"] < 0)
                o["term_step"][new], o["term_where"][new] = ts[new], tw[new]
            look(k + 1)
    o.update(in_band=below.any(0), crossings=np.abs(np.diff(below.astype(np.int8), axis=0)).sum(0), min_clr=min_clr, first_wow=first_wow)
    _ORACLE[key] = o
    return o


def coverage(o, groups, ok, label):
    """what the oracle alone says about the batch: does every instance behind this case get work, and is little of it excluded?"""
    live = o["status"] == 0
    wow, band = o["first_wow"] >= 0, o["in_band"]
    n_wave = (N + 63) // 64
    wave = np.arange(N) // 64
    per_wave = lambda m: np.bincount(wave[m], minlength=n_wave)
    excluded = {g: float((~ok | ~live)[m].mean()) for g, m in groups.items()}
    touched2 = float(wow[groups[2]].mean())
    crossed2 = float((o["crossings"] > 0)[groups[2]].mean())
    print(f"{label}: groups {[int(m.sum()) for m in groups.values()]}; below the band at some step {int(band.sum())}, crossed it {int((o['crossings'] > 0).sum())} "
          f"(group 2: {100 * crossed2:.0f} %), weight on wheels at some step {int(wow.sum())} (group 2: {100 * touched2:.1f} %); trim failures {int((~ok).sum())}, "
          f"terminated {int((~live).sum())}; excluded share per group {', '.join(f'{100 * v:.1f} %' for v in excluded.values())}")
    assert max(excluded.values()) <= 0.05, (label, excluded)
    # group 2 is what its name says — lanes that change pass and still hold the strict tolerance: a lane that touches down leaves the strict
    # comparison (the same 5 % cap as the excluded share), and at least half must go through the band's edge, not merely start inside it
    assert touched2 <= 0.05, (label, "group 2 must stay clear of the runway", touched2)
    assert crossed2 >= 0.5, (label, "group 2 must cross the band", crossed2)
    assert band.sum() >= N / 10 and wow.sum() >= N / 10, (label, int(band.sum()), int(wow.sum()))
    assert per_wave(band).min() >= 1 and per_wave(wow).min() >= 1 and per_wave(~band).min() >= 1, (label, "a wave without a lane of each kind")
    return wow


_DEVICE = {}


def device_run(fb, oracle, x2, kin, rows, duo, spl, dtype="f64"):
    key = (x2, kin, rows, duo, spl, dtype)
    if key in _DEVICE:
        return _DEVICE[key]
    K = fb.K
    sc = scenario(fb, oracle, x2, rows)
    with stepper(duo):
        w = fb.Cessna172Xv2World(N, gains=fb.ctl_gains.ctl_gains_blob(), kinematics=kin) if x2 else fb.BatchedWorld(N, kinematics=kin, dtype=dtype)
    if rows:
        w.env = sc["env6"]
        assert np.array_equal(w.env, sc["env6"])
    else:
        w.set_params(h_terrain=H_TRN)
    sim = fb.Simulation(w, dt=DT, Δt=DT * RATIO if x2 else None, save_on=False, steps_per_launch=spl)
    if x2:
        fb.init(sim, sc["tp"])
    else:
        fb.f_init(w, sc["tp"])
    ok = w.trim_success
    # the C ABI presents the mechanisation's own rows (fb_dims)
    nx = 18 + N_KIN[kin] + (K["FB_NACT"] if x2 else 0)
    assert w.nx == nx and w.x.shape == (nx, N)
    w.set_state(sc["perturb"](w.x, kin), w.s)
    if x2:
        w.cu = sc["set_cu"](w.cu)
    start = dict(x=w.x, s=w.s, u=w.u, ui=w.ui)
    if x2:
        start.update(cu=w.cu, cs=w.cs)
    fb.step(sim, NSTEPS * DT); w.sync()
    tstep, twhere = w.termination
    r = dict(start=start, ok=ok, x=w.x, s=w.s, status=w.status, tstep=tstep, twhere=twhere)
    if x2:
        r.update(cu=w.cu, cs=w.cs)
    # fb_get_state / fb_set_state round trip of the END state (ϕ, λ, ψ far from zero, actuator block present): every row, bit for bit
    w.set_state(r["x"], r["s"])
    assert np.array_equal(w.x, r["x"]) and np.array_equal(w.s, r["s"]), "state does not round-trip through the C ABI"
    w.close()
    _DEVICE[key] = r
    return r


def reference(fb, oracle, x2, kin, rows, dev, label):
    """the oracle's run from the device's start state, its coverage, and — with rows — the proof that the rows decide the result"""
    sc = scenario(fb, oracle, x2, rows)
    env = oracle.env_rows(sc["env6"]) if rows else oracle.default_env(h_trn=H_TRN)
    ok = oracle_trim_ok(fb, oracle, x2, kin, rows)
    assert np.array_equal(ok, dev["ok"]), f"{label}: device and oracle trims disagree on {int((ok != dev['ok']).sum())} aircraft"
    o = oracle_run(fb, oracle, x2, kin, env, dev["start"], sc["h_trn"], sc["N0"])
    wow = coverage(o, sc["groups"], ok, label)
    if rows:
        rows_matter(fb, oracle, x2, kin, dev["start"], sc, o, ok, label)
    return o, wow, ok


def rows_matter(fb, oracle, x2, kin, start, sc, o, ok, label):
    """the same start state in the batch-wide default block (what a kernel that ignored the rows would fly in): at least 1000 x the
    tolerance away on every airborne lane, and no touchdown, or one at another step, where the per-aircraft terrain gives one"""
    flat = oracle_run(fb, oracle, x2, kin, oracle.default_env(), start, np.zeros(N), sc["N0"])
    live = ok & (o["status"] == 0)
    air = live & (o["first_wow"] < 0) & (flat["status"] == 0)
    d = (np.abs(flat["x"] - o["x"]) / state_scale(o["x"], kin)).max(0)
    touched = ok & (o["first_wow"] >= 0)
    print(f"{label}: without the rows: airborne lanes differ by {d[air].min():.2e} .. {d[air].max():.2e}; of {int(touched.sum())} that touch down, "
          f"{int((flat['first_wow'][touched] < 0).sum())} never do and {int((flat['first_wow'] == o['first_wow'])[touched].sum())} do so at the same step")
    assert d[air].min() >= 1000 * TOL, (label, d[air].min())
    assert ((flat["first_wow"] != o["first_wow"]) | (flat["status"] != o["status"]))[touched].all(), label


def compare(fb, x2, kin, dev, o, wow, ok, label):
    """status words and termination record on every aircraft; discrete states on the live ones; airborne lanes at the strict
    tolerance, lanes that had weight on wheels in altitude and attitude"""
    K = fb.K
    rmap = abi_to_oracle_rows(K, "x2" if x2 else "s0", kin)
    assert np.array_equal(dev["status"], o["status"]), f"{label}: {int((dev['status'] != o['status']).sum())} status words differ"
    assert np.array_equal(dev["tstep"], o["term_step"]) and np.array_equal(dev["twhere"], o["term_where"]), f"{label}: termination record"
    live = o["status"] == 0
    assert np.array_equal(dev["s"][:, live], o["s"][:, live]), f"{label}: discrete states differ"
    xo = o["x"][rmap]
    err = (np.abs(dev["x"] - xo) / state_scale(o["x"], kin)[rmap]).max(0)
    cerr = (np.abs(dev["cs"] - o["cs"]) / np.maximum(np.abs(o["cs"]), 1.0)).max(0) if x2 else np.zeros(N)
    strict, ground = ok & live & ~wow, ok & live & wow
    hr = int(np.nonzero(rmap == H_E_ROW[kin])[0][0])
    att = [int(np.nonzero(rmap == r)[0][0]) for r in range(ATT[kin].start, ATT[kin].stop)]
    dh, dq = np.abs(dev["x"][hr] - xo[hr]), np.abs(dev["x"][att] - xo[att]).max(0)
    print(f"{label}: worst scaled error on {int(strict.sum())} airborne lanes: state {err[strict].max():.2e}, control-law record {cerr[strict].max():.2e}; "
          f"on {int(ground.sum())} lanes in ground contact: altitude {dh[ground].max():.2e} m, attitude {dq[ground].max():.2e}")
    assert err[strict].max() < TOL, (label, err[strict].max(), int(np.nonzero(strict)[0][err[strict].argmax()]))
    assert cerr[strict].max() < TOL, (label, cerr[strict].max())
    if x2:
        assert np.array_equal(dev["cu"][:, strict], o["cu"][:, strict]), f"{label}: control-law inputs differ"
    assert dh[ground].max() < TOL_GROUND and dq[ground].max() < TOL_GROUND, (label, dh[ground].max(), dq[ground].max())


MATRIX = [(x2, kin, rows, duo) for x2 in (False, True) for kin in ("WA", "ECEF", "NED") for rows in (False, True) for duo in (True, False)]


def launch_length(x2, kin, rows, duo):
    """7 or 50 steps per launch, alternating along every axis of the matrix"""
    return 7 if (int(x2) + ("WA", "ECEF", "NED").index(kin) + int(rows) + int(duo)) % 2 == 0 else 50


def case_id(x2, kin, rows, duo):
    return f"{'Xv2' if x2 else 'Sv0'}-{kin}-{'rows' if rows else 'block'}-{'duo' if duo else 'air'}"


@pytest.mark.parametrize("x2,kin,rows,duo", MATRIX, ids=[case_id(*c) for c in MATRIX])
def test_stepping_instance_against_oracle(fb, oracle, x2, kin, rows, duo):
    spl = launch_length(x2, kin, rows, duo)
    label = f"{case_id(x2, kin, rows, duo)} ({spl} steps per launch)"
    dev = device_run(fb, oracle, x2, kin, rows, duo, spl)
    o, wow, ok = reference(fb, oracle, x2, kin, rows, dev, label)
    compare(fb, x2, kin, dev, o, wow, ok, label)


def test_f32_handle_without_rows_runs_the_fp32_stepper(fb, oracle):
    """FB_F32 handle, batch-wide block: fbf::k_step_f32 on the airborne lanes, held to the fp32 bounds (tests/test_gpu_f32.py) on group 1;
    groups 2 and 3 are handed to the fp64 ground-capable instance after an fp32 approach: altitude and status, as
    test_f32_hands_ground_contact_to_the_fp64_kernel holds them."""
    label = "f32-block (50 steps per launch)"
    dev = device_run(fb, oracle, False, "WA", False, True, 50, dtype="f32")
    o, wow, ok = reference(fb, oracle, False, "WA", False, dev, label)
    g = scenario(fb, oracle, False, False)["groups"]
    g1 = g[1] & ok & (o["status"] == 0)
    assert (dev["status"][g1] == 0).all() and np.array_equal(dev["s"][:, g1], o["s"][:, g1])
    d = np.abs(dev["x"] - o["x"])[:, g1]
    tol = F32_TOLERANCE
    print(f"{label}: group 1 ({int(g1.sum())} lanes): rates {d[21:24].max():.1e} rad/s, velocity {d[24:27].max():.1e} m/s, altitude {d[20].max():.1e} m, "
          f"q_wb {d[12:16].max():.1e}, q_ew {d[16:20].max():.1e}, engine speed {d[9].max():.1e} rad/s")
    assert d[21:24].max() < tol["rates_rad_s"] and d[24:27].max() < tol["velocity_m_s"] and d[20].max() < tol["altitude_m"]
    assert d[12:16].max() < tol["q_wb"] and d[9].max() < tol["engine_speed_rad_s"] and d[16:20].max() < tol["q_ew"]
    # ... and it WAS the fp32 stepper: k_step_duo<WA, false, false> on this handle would meet every bound above. 500 steps of fp32
    # arithmetic (unit round-off 6e-8) leave every lane far from the fp64 handle's result (the Sv0-WA-block-duo case: same batch, same
    # launch length); two fp64 steppers differ by accumulated fp64 rounding, orders below 1e-10
    f64 = device_run(fb, oracle, False, "WA", False, True, 50)
    assert np.array_equal(f64["start"]["x"], dev["start"]["x"])
    apart = (np.abs(dev["x"] - f64["x"]) / state_scale(f64["x"], "WA")).max(0)[g1]
    print(f"{label}: group 1 against the fp64 handle: scaled distance {apart.min():.1e} .. {apart.max():.1e}")
    assert apart.min() > 1e-10, "an FB_F32 handle without rows was stepped in fp64"
    near = (g[2] | g[3]) & ok
    live = near & (o["status"] == 0) & (dev["status"] == 0)
    h_err = np.abs(dev["x"][20] - o["x"][20])[live]
    print(f"{label}: groups 2 and 3: {int(live.sum())} of {int(near.sum())} live on both sides, status words differ on {int((dev['status'] != o['status'])[near].sum())}; "
          f"altitude: median {np.median(h_err):.1e} m, worst {h_err.max():.1e} m")
    assert live.sum() > 0.9 * near.sum()
    assert np.median(h_err) < 0.05 and h_err.max() < 1.0


def test_f32_handle_with_rows_runs_the_fp64_one_wave_kernel(fb, oracle):
    """FB_F32 handle with per-aircraft rows: the fp32 stepper has no such form, the handle is stepped by k_step_air<WA, false, false, true> —
    the very kernel of the FLIGHTBATCH_DUO=0 fp64 handle, bit for bit (and that one is held to the oracle in Sv0-WA-rows-air)."""
    spl = launch_length(False, "WA", True, False)
    f32 = device_run(fb, oracle, False, "WA", True, True, spl, dtype="f32")
    f64 = device_run(fb, oracle, False, "WA", True, False, spl)
    assert np.array_equal(f32["start"]["x"], f64["start"]["x"])
    print(f"f32-rows ({spl} steps per launch): {int((f32['status'] != 0).sum())} terminated; states differ on {int((f32['x'] != f64['x']).any(0).sum())} aircraft")
    assert np.array_equal(f32["x"], f64["x"]) and np.array_equal(f32["s"], f64["s"]) and np.array_equal(f32["status"], f64["status"])
    assert np.array_equal(f32["tstep"], f64["tstep"]) and np.array_equal(f32["twhere"], f64["twhere"])
