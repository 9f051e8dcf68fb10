"""The batch that holds the fp32 airborne stepper (fbf::k_step_f32, csrc/c172_kernels_f32.hpp) to the oracle: host-only inputs, the oracle's
histories of them, the perturbed oracle runs that show the batch to be FAIR for an fp32 kernel, and the one helper that runs it on a handle.
No device work at import; tests/test_f32_cases_host.py (CPU) proves what the device tests (test_gpu_f32_events.py, test_gpu_f32_edges.py) rely on.

Lane k is of kind k % 12. Kinds 0-7 are tests/golden/make_duo_stage_pin.py's (make_inputs is imported, not copied: a pool of its lanes is
formed and lanes of the wanted kind are drawn from it in order); kinds 8-11 are cruise lanes of that pool, changed here:

     8  engine running, FB_UI_ENG_STOP set: off at the first f_step!
     9  engine off, FB_UI_ENG_START set, engine speed 20-60 rad/s: off -> starting at step 1, running within 5-40 steps
    10  running dry: 1e-6 .. 2e-6 of fuel at the start, so the engine goes off at steps 2 .. 12 (below 1e-6 some go off at the first step)
    11  level flight 5 m above the terrain (h_terrain = 0: the geoid) for the whole run: inside the hand-over band from the first evaluation
        of every launch, the fp32 kernel never commits it
    8 and 11, every second lane: one friction-regulator state non-zero at the start (the `to_ground` branch of the kernel's prologue)

n = 76 is a full wave and a ragged one of twelve lanes (one of each kind); n = 268 puts a ragged wave into a second 256-lane workgroup."""
import ctypes as C

import numpy as np

from golden import make_duo_stage_pin as pin
from support import state_scale, stepper

DT = pin.DT
NKIND, SIZES, LENGTHS = 12, (76, 268), (14, 100)
PARTITIONS = {14: (1, 2, 7, 14), 100: (50, 7)}       # steps per launch, per run length
K_DRAWS, REL_DRAW = 12, 2.0 ** -19                    # conditioning: draws per size and length; relative size of a draw (about 32 fp32 ulps)
K_ENVELOPE = 6                                        # oracle runs behind the envelope
FACTOR = 10.0                                         # the family's factor on an envelope (conditioning.py; FACTOR of the linear family)
BAND = 10.0                                           # [m] clearance over the terrain below which an airborne kernel hands a lane over
FUEL_DRY = (1e-6, 2e-6)                               # kind 10: the engine goes off at steps 2 .. 12 (a cruise lane burns 3.5e-7 .. 7.3e-7 per step)
LEVEL_CLEARANCE = 5.0
F32_ROWS = np.array([r for r in range(27) if not (2 <= r < 8) and not (16 <= r < 21)])    # the sixteen rows the kernel holds in fp32
assert F32_ROWS.size == 16

_INPUTS, _HIST, _COND, _ENV = {}, {}, {}, {}


def make_inputs(K, orc, n):
    """dict: x0, s0, u, ui, st0, lat, lon, kind, to_ground (computed once per size, shared, never modified)"""
    if n in _INPUTS:
        return _INPUTS[n]
    per = -(-n // NKIND)                                      # lanes of a kind, at the most
    m = 8 * (5 * per + 1)                                     # the pool: cruise lanes for kinds 0, 8, 9, 10, 11; one spare kind-6 lane
    px, ps, pu, pui, pst, plat, plon = pin.make_inputs(K, orc, m)
    pool_kind = np.arange(m) % 8
    kind = np.arange(n) % NKIND
    src = np.zeros(n, np.int64)
    cruise = np.flatnonzero(pool_kind == 0)
    for k in range(NKIND):
        lanes = np.flatnonzero(kind == k)
        if k < 8:
            cand = np.flatnonzero(pool_kind == k)
            if k == 6:      # dead, live, dead, ... in the pool: start at a live one, so that the ragged last wave (lane index 5, 21 of the kind) gets a dead one
                cand = cand[1:]
            src[lanes] = cruise[:lanes.size] if k == 0 else cand[:lanes.size]
        else:
            src[lanes] = cruise[(k - 7) * per:(k - 7) * per + lanes.size]
    assert np.unique(src).size == n
    x, s, u, ui, st0, lat, lon = (np.ascontiguousarray(a[..., src]) for a in (px, ps, pu, pui, pst, plat, plon))
    rng = np.random.default_rng(20261020 + 1000 * n)
    cnt = lambda k: int((kind == k).sum())
    ENG, FUEL, W = K["FB_S_ENG_STATE"], K["FB_X_FUEL"], K["FB_X_ENG_OMEGA"]
    w_idle = 600 * np.pi / 30
    x[W, kind == 4] = w_idle - 0.85 * (w_idle - x[W, kind == 4])      # 17 .. 25.5 rad/s below idle: the slowest is running before the last of 14 steps
    ui[kind == 8] |= K["FB_UI_ENG_STOP"]
    s[ENG, kind == 9] = 0
    ui[kind == 9] |= K["FB_UI_ENG_START"]
    x[W, kind == 9] = rng.uniform(20.0, 60.0, cnt(9))
    x[FUEL, kind == 10] = np.exp(rng.uniform(np.log(FUEL_DRY[0]), np.log(FUEL_DRY[1]), cnt(10)))
    k11 = kind == 11
    x[K["FB_X_H_E"], k11] = pin.geoid(orc, lat[k11], lon[k11]) + LEVEL_CLEARANCE
    to_ground = ((kind == 8) | k11) & ((np.arange(n) // NKIND) % 2 == 1)
    frc = K["FB_X_LDG_FRC"] + (np.arange(n) // NKIND) % 6
    x[frc[to_ground], np.flatnonzero(to_ground)] = rng.uniform(0.05, 0.3, int(to_ground.sum())) * rng.choice([-1.0, 1.0], int(to_ground.sum()))
    for a in (x, s, u, ui, st0, lat, lon, kind, to_ground):
        a.setflags(write=False)
    _INPUTS[n] = dict(x0=x, s0=s, u=u, ui=ui, st0=st0, lat=lat, lon=lon, kind=kind, to_ground=to_ground, geoid=pin.geoid(orc, lat, lon))
    return _INPUTS[n]


def oracle_history(orc, inp, nsteps, x0=None, jitter_rng=None):
    """the oracle one step at a time: dict of x [nsteps+1, 27, n], s [nsteps+1, 2, n], status [nsteps+1, n] after 0 .. nsteps steps and the
    termination record. jitter_rng: every fp32-held row moved by one fp32 ulp of its own value after every step, direction drawn per row,
    lane and step (the envelope's runs)."""
    n = inp["x0"].shape[1]
    x = np.array(inp["x0"] if x0 is None else x0, copy=True); s = np.array(inp["s0"], copy=True); st = np.array(inp["st0"], copy=True)
    X, S, ST = [x.copy()], [s.copy()], [st.copy()]
    tstep, twhere = np.full(n, -1, np.int64), np.zeros(n, np.int32)
    env = orc.default_env()
    for k in range(nsteps):
        x, s, st, ts, tw = orc.step_term(x, inp["u"], inp["ui"], s, env, DT, 1, step0=k, status=st)
        new = (ts >= 0) & (tstep < 0)
        tstep[new], twhere[new] = ts[new], tw[new]
        if jitter_rng is not None:
            live = st == 0
            ulp = np.spacing(np.abs(x[F32_ROWS]).astype(np.float32)).astype(np.float64)
            x[F32_ROWS] = np.where(live, x[F32_ROWS] + ulp * jitter_rng.choice([-1.0, 1.0], ulp.shape), x[F32_ROWS])
        X.append(x.copy()); S.append(s.copy()); ST.append(st.copy())
    return dict(x=np.stack(X), s=np.stack(S), status=np.stack(ST), term_step=tstep, term_where=twhere)


def history(K, orc, n, nsteps):
    """the unperturbed oracle history of a size and length (cached, shared, left unchanged)"""
    if (n, nsteps) not in _HIST:
        _HIST[n, nsteps] = oracle_history(orc, make_inputs(K, orc, n), nsteps)
    return _HIST[n, nsteps]


def conditioning_runs(K, orc, n, nsteps):
    """K_DRAWS + 1 histories from start states an fp32 kernel cannot tell apart: the fp32-held rows rounded to float32 (run 0), then moved by a
    relative uniform ±REL_DRAW; q_ew and h_e stay as they are"""
    if (n, nsteps) not in _COND:
        inp = make_inputs(K, orc, n)
        rng = np.random.default_rng(7 * n + nsteps)
        runs = []
        for k in range(K_DRAWS + 1):
            x0 = np.array(inp["x0"], copy=True)
            x0[F32_ROWS] = x0[F32_ROWS].astype(np.float32).astype(np.float64) if k == 0 else x0[F32_ROWS] * (1 + rng.uniform(-REL_DRAW, REL_DRAW, (16, n)))
            runs.append(oracle_history(orc, inp, nsteps, x0=x0))
        _COND[n, nsteps] = runs
    return _COND[n, nsteps]


def scaled_error(x, xo):
    """per-lane maximum over the rows of |x - xo| / support.state_scale(xo)"""
    return (np.abs(x - xo) / state_scale(xo)).max(0)


def envelope(K, orc, n, nsteps):
    """E [K_ENVELOPE, n]: per-lane maximum scaled |oracle' - oracle| after nsteps, oracle' stepped with one fp32 ulp of jitter per step on every
    fp32-held row"""
    if (n, nsteps) not in _ENV:
        ref = history(K, orc, n, nsteps)["x"][nsteps]
        rng = np.random.default_rng(11 * n + nsteps)
        _ENV[n, nsteps] = np.stack([scaled_error(oracle_history(orc, make_inputs(K, orc, n), nsteps, jitter_rng=rng)["x"][nsteps], ref)
                                    for _ in range(K_ENVELOPE)])
    return _ENV[n, nsteps]


def clearance(K, inp, hist):
    """[nsteps+1, n] height of the body origin over the terrain (h_terrain = 0: the geoid)"""
    return hist["x"][:, K["FB_X_H_E"]] - inp["geoid"]


def lane_sets(K, inp, hist):
    """dead: terminated before the launch; airborne: live in the oracle to the end, never within BAND + 1 m of the terrain and no regulator state
    set (the fp32 kernel commits every step of theirs); banded: kind 11 (never committed by it)"""
    dead = inp["st0"] != 0
    airborne = ~dead & (hist["status"][-1] == 0) & (clearance(K, inp, hist).min(0) > BAND + 1.0) & ~inp["to_ground"]
    return dead, airborne, inp["kind"] == 11


def never_committed(K, inp, hist, spl):
    """lanes no launch of the fp32 kernel commits when the run is cut into launches of spl steps: terminated before the run, within the band at
    every launch start (kind 11), or a regulator state non-zero at every launch start (the oracle says whether f_step! has reset it by then)"""
    nsteps = hist["x"].shape[0] - 1
    starts = np.arange(0, nsteps, spl)
    frc = hist["x"][starts, K["FB_X_LDG_FRC"]:K["FB_X_LDG_FRC"] + 6]
    return (inp["st0"] != 0) | (inp["kind"] == 11) | (inp["to_ground"] & (frc != 0).any(1).all(0))


def first_step(flags):
    """[nsteps+1, n] bool -> the first index at which a lane's flag holds, -1 where it never does"""
    return np.where(flags.any(0), flags.argmax(0), -1)


# ---- the device side -----------------------------------------------------------------------------------------------------------------------
def run_device(fb, inp, nsteps, spl, dtype="f32", duo=True, lanes=None, every_launch=False):
    """the batch (or its lanes `lanes`, in that order) on a fresh handle, nsteps in launches of spl. Returns dict x, s, status, term_step, term_where;
    with every_launch also hist_s [launches+1, 2, n] and hist_status [launches+1, n], read after every launch."""
    sel = np.arange(inp["x0"].shape[1]) if lanes is None else np.asarray(lanes)
    x0, s0, u, ui, st0 = (np.ascontiguousarray(inp[k][..., sel]) for k in ("x0", "s0", "u", "ui", "st0"))
    with stepper(duo):
        w = fb.BatchedWorld(sel.size, dtype=dtype)
    try:
        w.set_state(x0, s0); w.u = u; w.ui = ui
        fb._lib.check(fb.lib.fb_set_status(w._h, st0.ctypes.data_as(C.POINTER(C.c_int32))))
        sim = fb.Simulation(w, dt=DT, save_on=False, steps_per_launch=spl)
        out = {}
        if every_launch:
            hs, hst = [w.s], [w.status]
            for k in range(0, nsteps, spl):
                fb.step(sim, min(spl, nsteps - k) * DT); w.sync()
                hs.append(w.s); hst.append(w.status)
            out.update(hist_s=np.stack(hs), hist_status=np.stack(hst))
        else:
            fb.step(sim, nsteps * DT); w.sync()
        ts, tw = w.termination
        out.update(x=w.x, s=w.s, status=w.status, term_step=ts, term_where=tw)
        return out
    finally:
        w.close()


def same_words(a, b, lanes=slice(None)):
    """x (as bits: the sign of a zero counts), s, status and the termination record of two runs equal on `lanes`"""
    return (np.array_equal(a["x"][:, lanes].view(np.uint64), b["x"][:, lanes].view(np.uint64)) and np.array_equal(a["s"][:, lanes], b["s"][:, lanes])
            and np.array_equal(a["status"][lanes], b["status"][lanes]) and np.array_equal(a["term_step"][lanes], b["term_step"][lanes])
            and np.array_equal(a["term_where"][lanes], b["term_where"][lanes]))
