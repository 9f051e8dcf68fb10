"""Scripted scenarios as a table: the device-side `user_callback!`.

The reference's scenarios are closures handed to `Simulation(...; user_callback!)` that run after every step (lib/FlightCore/src/sim.jl:185,
334-336): a `phase` symbol, and per phase "set these inputs; if <condition on the model's outputs> then set those inputs and go to the next
phase" (lib/FlightApps/demos/c172_demos.jl:423-486 crosswind landing, :525-642 traffic pattern). A batch of N simulations cannot call back into
the host after every step without crossing PCIe with the whole output record; the same logic as DATA — phases, rules, actions — is evaluated
on the device by `k_scenario` (csrc/scenario_kernels.hpp) between the stepping launches, with one phase word, one entry time, `n_par`
parameters and `n_rec` record slots per aircraft. Nothing of a run touches the host.

    scn = Scenario(n_par=..., n_rec=...)
    FINAL, FLARE = scn.phase("final"), scn.phase("flare")
    scn.when(FINAL, src.H_E - par(P_H_RWY) < 6.0, [cu("SEG_VRT_REQ", 0), cu("CLM_REF", -0.3), ...], then=FLARE)
    scn.always(GROUND, [cu("THROTTLE_AXIS", 0), u("BRAKE_LEFT", 1)])
    world.set_scenario(scn, params=[n_par, n], every=1)

Semantics of one evaluation (one aircraft): the `always` actions of its phase run; then the phase's rules are tried in order and the FIRST whose
condition holds runs its actions and sets the next phase — at most one transition per evaluation, as in the demos' if / elseif chains.
Values are read when their action runs, so an action sees what the actions before it wrote.

Models. The reference's callback runs on whatever model the Simulation holds (sim.jl:279), and its first Cessna172Sv0 demos are scripted input
changes (nlsim_q, nlsim_θ: one second from trim, then `act.u.elevator += 0.1`, c172_demos.jl:108-206). A table loads on a `Cessna172Xv2World` and on
a `BatchedWorld` (Cessna172Sv0, fp64, any mechanisation); the second has no control-law rows, so cs_ / cu_ sources and cu destinations are refused
there — by the library when the table is loaded, and by `pack(model="Cessna172Sv0")` before it gets that far. Its scripts write `u(...)`, `ui(...)`
and `rec(...)` and read T, T_IN_PHASE, x_ (27 rows), u_, s_, ON_GND, H_E, PSI, THETA, PHI, CHI, EAS, CLM, par, rec_.

The world. The reference's scripts set `world.atmosphere.wind.u.N / .E` as well (c172_demos.jl:225-228, 427-433) and may read anything in `mdl.y`
(sim.jl:185, 279, 334-336). On a world whose per-aircraft environment rows are set (`set_env`), `env_("WIND_E")` reads the aircraft's own row (all six
FB_ENV_* rows) and `env("WIND_E", value)` writes its wind (the three wind rows only: the sea-level rows carry derived rows only the host computes, the
terrain elevation is a constructor argument in the reference); `y_(row)` reads any row of the output record at the state behind the step — the device
then refreshes the whole record ahead of every evaluation, one `f_ode!` pass that a table without `y_` does not pay.

`evaluate_on_host` is the same interpreter in numpy over arrays the caller supplies: the host-callback form of a table (tests compare the two),
and the checker's phase machine in tests/test_gpu_scenarios.py (driving the CPU oracle). `host_callback` wraps it as the `user_callback` of a
Simulation: the model's arrays down, one evaluation, what changed back up."""
from __future__ import annotations

import numpy as np

from ._lib import K

MAGIC = 5.0e6 + 1   # version 1 of the blob layout
HDR, PH_REC, RULE_REC, ACT_REC, NTERM = 8, 4, 8, 14, 3
# value sources (kind, row)
SRC = {name: K["FB_SCN_SRC_" + name] for name in ("CONST", "T", "T_IN_PHASE", "X", "CS", "CU", "U", "S", "ON_GND", "H_E", "PSI", "THETA", "PHI", "CHI",
                                                     "EAS", "CLM", "PAR", "REC", "ENV", "Y")}
DST = {name: K["FB_SCN_DST_" + name] for name in ("CU", "U", "UI", "REC", "ENV")}
WIND_ROWS = (K["FB_ENV_WIND_N"], K["FB_ENV_WIND_E"], K["FB_ENV_WIND_D"])
TAPPED = tuple(SRC[k] for k in ("ON_GND", "H_E", "PSI", "THETA", "PHI", "CHI", "EAS", "CLM"))
CMP = {"<": K["FB_SCN_LT"], ">": K["FB_SCN_GT"], ">=": K["FB_SCN_GE"], "<=": K["FB_SCN_LE"], "==": K["FB_SCN_EQ"], "!=": K["FB_SCN_NE"], "always": K["FB_SCN_ALWAYS"]}


class Value:
    """c0 + sum of up to three coefficient x source terms, optionally wrapped to (-pi, pi] (Attitude.wrap_to_π, FP/attitude.jl:478)"""

    def __init__(self, c0=0.0, terms=(), wrap=False):
        self.c0, self.terms, self.wrap = float(c0), tuple(terms), bool(wrap)
        if len(self.terms) > NTERM:
            raise ValueError(f"a scenario value holds at most {NTERM} terms")

    def _lift(self, o):
        return o if isinstance(o, Value) else Value(float(o))

    def __add__(self, o):
        o = self._lift(o)
        return Value(self.c0 + o.c0, self.terms + o.terms, self.wrap or o.wrap)

    __radd__ = __add__

    def __neg__(self):
        return Value(-self.c0, tuple((k, r, -c) for k, r, c in self.terms), self.wrap)

    def __sub__(self, o):
        return self + (-self._lift(o))

    def __rsub__(self, o):
        return self._lift(o) + (-self)

    def __mul__(self, c):
        return Value(self.c0 * c, tuple((k, r, cc * c) for k, r, cc in self.terms), self.wrap)

    __rmul__ = __mul__

    # comparisons build conditions: one plain source, optionally minus one parameter row, against a constant:
    #     src.H_E - par(7) < 6.0        cs_("SEG_S_2B") > -200.0
    # (evaluated as written — lhs - par, then the comparison — like `vehicle.y.kinematics.h_e - final_leg.p2.h < 6` in the demos)
    def _cond(self, op, o):
        o = self._lift(o)
        if o.terms or o.wrap or self.wrap or self.c0 != 0.0:
            raise ValueError("a scenario condition compares `source [- par(row)]` with a constant")
        plain = [t for t in self.terms if t[0] != SRC["PAR"]]
        pars = [t for t in self.terms if t[0] == SRC["PAR"]]
        if len(plain) != 1 or plain[0][2] != 1.0 or len(pars) > 1 or (pars and pars[0][2] != -1.0):
            raise ValueError("a scenario condition compares `source [- par(row)]` with a constant")
        return Condition(plain[0][0], plain[0][1], CMP[op], o.c0, pars[0][1] if pars else -1)

    def __lt__(self, o): return self._cond("<", o)
    def __gt__(self, o): return self._cond(">", o)
    def __ge__(self, o): return self._cond(">=", o)
    def __le__(self, o): return self._cond("<=", o)
    def eq(self, o): return self._cond("==", o)
    def ne(self, o): return self._cond("!=", o)


def wrap_to_pi(v: Value) -> Value:
    return Value(v.c0, v.terms, True)


class Condition:
    def __init__(self, kind, row, cmp, thr, thr_par=-1):
        self.kind, self.row, self.cmp, self.thr, self.thr_par = int(kind), int(row), int(cmp), float(thr), int(thr_par)


ALWAYS = Condition(SRC["CONST"], 0, CMP["always"], 0.0)


def _src(kind, row=0):
    return Value(0.0, ((SRC[kind], int(row), 1.0),))


class _Sources:
    """src.T, src.H_E, src.PSI, src.ON_GND, ...: what a condition or a value may read of the model after a step"""
    T = _src("T"); T_IN_PHASE = _src("T_IN_PHASE"); ON_GND = _src("ON_GND"); H_E = _src("H_E"); PSI = _src("PSI"); THETA = _src("THETA")
    PHI = _src("PHI"); CHI = _src("CHI"); EAS = _src("EAS"); CLM = _src("CLM")


src = _Sources()


def cs_(name_or_row) -> Value:
    """a row of the control-law record (avionics.y): cs_('SEG_S_2B')"""
    return _src("CS", K["FB_CS_" + name_or_row] if isinstance(name_or_row, str) else name_or_row)


def cu_(name_or_row) -> Value:
    return _src("CU", K["FB_CU_" + name_or_row] if isinstance(name_or_row, str) else name_or_row)


def u_(name_or_row) -> Value:
    """a row of the vehicle's inputs (FB_U_*): u("ELEVATOR", u_("ELEVATOR") + par(0)) is `act.u.elevator += a`"""
    return _src("U", K["FB_U_" + name_or_row] if isinstance(name_or_row, str) else name_or_row)


def x_(row) -> Value:
    """a row of the continuous state, in the device's row order (include/flightbatch.h)"""
    return _src("X", row)


def s_(name_or_row) -> Value:
    """a discrete state row (FB_S_STALL, FB_S_ENG_STATE)"""
    return _src("S", K["FB_S_" + name_or_row] if isinstance(name_or_row, str) else name_or_row)


def _env_row(name_or_row) -> int:
    return K["FB_ENV_" + name_or_row] if isinstance(name_or_row, str) else int(name_or_row)


def env_(name_or_row) -> Value:
    """a row of the aircraft's own environment (FB_ENV_*: env_("WIND_E"), env_("H_TERRAIN")), as world.env holds it; the world needs rows (set_env)"""
    return _src("ENV", _env_row(name_or_row))


def y_(row) -> Value:
    """a row of the output record mdl.y at the state behind the step (include/flightbatch.h FB_Y_*: y_(K["FB_Y_AIR"] + 19) is the TAS)"""
    return _src("Y", K[row] if isinstance(row, str) else row)


def par(row) -> Value:
    return _src("PAR", row)


def rec_(row) -> Value:
    return _src("REC", row)


class Action:
    def __init__(self, dst, row, value):
        self.dst, self.row = int(dst), int(row)
        self.value = value if isinstance(value, Value) else Value(float(value))


def cu(name, value) -> Action:
    """avionics.{gdc, ctl}.u.<field> = value (a row of the control-law inputs, FB_CU_*)"""
    return Action(DST["CU"], K["FB_CU_" + name], value)


def u(name, value) -> Action:
    """a row of the vehicle's inputs (FB_U_*: flaps, brakes, ...)"""
    return Action(DST["U"], K["FB_U_" + name], value)


def ui(bit_name, on) -> Action:
    """a bit of the discrete inputs (FB_UI_*: engine start / stop ...): set where value != 0, cleared otherwise"""
    return Action(DST["UI"], K["FB_UI_" + bit_name], on if isinstance(on, Value) else (1.0 if on else 0.0))


def rec(row, value) -> Action:
    """record slot `row` of the aircraft = value (touchdown time, position ...: read back with world.scenario_state())"""
    return Action(DST["REC"], row, value)


def env(name, value) -> Action:
    """world.atmosphere.wind.u.<N / E / D> = value for this aircraft (FB_ENV_WIND_N / _E / _D; the other environment rows are refused by pack)"""
    return Action(DST["ENV"], _env_row(name), value)


def target(p1_par: int, p2_par: int):
    """gdc.seg.u.target = Segment(p1, p2) with the end points in parameter rows p1_par .. p1_par + 2, p2_par .. p2_par + 2"""
    return [Action(DST["CU"], K["FB_CU_SEG_P1"] + k, par(p1_par + k)) for k in range(3)] + [Action(DST["CU"], K["FB_CU_SEG_P2"] + k, par(p2_par + k)) for k in range(3)]


class Scenario:
    def __init__(self, n_par=0, n_rec=0):
        self.n_par, self.n_rec = int(n_par), int(n_rec)
        self.names: list[str] = []
        self._always: list[list[Action]] = []
        self._rules: list[list[tuple]] = []

    def phase(self, name: str) -> int:
        self.names.append(name); self._always.append([]); self._rules.append([])
        return len(self.names) - 1

    def always(self, phase: int, actions):
        self._always[phase] += list(actions)

    def when(self, phase: int, cond: Condition, actions=(), then: int | None = None):
        self._rules[phase].append((cond, list(actions), phase if then is None else int(then)))

    def pack(self, model: str | None = None) -> np.ndarray:
        """the FB_TABLE_SCENARIO blob (include/flightbatch.h). model="Cessna172Sv0": raise on what that model lacks (control-law rows as sources or
        destinations, state rows past its 27) instead of leaving it to the library; the blob is the same either way."""
        if model not in (None, "Cessna172Sv0", "Cessna172Xv2"):
            raise ValueError(f"Scenario.pack: unknown model {model!r}")
        if model == "Cessna172Sv0":
            reads = [(c.kind, c.row) for p in self._rules for c, _, _ in p]
            every = [a for p in self._always for a in p] + [a for p in self._rules for _, ra, _ in p for a in ra]
            reads += [(k, r) for a in every for k, r, _ in a.value.terms]
            if any(k in (SRC["CS"], SRC["CU"]) for k, _ in reads) or any(a.dst == DST["CU"] for a in every):
                raise ValueError("the table addresses control-law rows (cs_ / cu_ sources, cu destinations), which only a Cessna172Xv2 has")
            if any(k == SRC["X"] and not 0 <= r < K["FB_NX"] for k, r in reads):
                raise ValueError(f"a Cessna172Sv0 has {K['FB_NX']} state rows")
        all_reads = [(c.kind, c.row) for p in self._rules for c, _, _ in p]
        all_acts = [a for p in self._always for a in p] + [a for p in self._rules for _, ra, _ in p for a in ra]
        all_reads += [(k, r) for a in all_acts for k, r, _ in a.value.terms]
        for k, r in all_reads:   # (what the library refuses when the table is loaded, whatever the model)
            if k == SRC["ENV"] and not 0 <= r < K["FB_NENV"]:
                raise ValueError(f"environment row out of range: the rows are FB_ENV_* (0 .. {K['FB_NENV'] - 1})")
            if k == SRC["Y"] and not 0 <= r < K["FB_NY"]:
                raise ValueError(f"output row out of range: the output record has {K['FB_NY']} rows")
        for a in all_acts:
            if a.dst != DST["ENV"]:
                continue
            if a.row in (K["FB_ENV_T_SL"], K["FB_ENV_P_SL"]):
                raise ValueError("a table cannot write the sea-level rows (T_SL, P_SL): each carries derived rows the host fills with its own log / exp / sqrt "
                                 "(set_env), which a device write could not reproduce; a table writes WIND_N / WIND_E / WIND_D")
            if a.row == K["FB_ENV_H_TERRAIN"]:
                raise ValueError("a table cannot write H_TERRAIN: the terrain elevation is a constructor argument of HorizontalTerrain in the reference, not an "
                                 "input; a table writes WIND_N / WIND_E / WIND_D")
            if a.row not in WIND_ROWS:
                raise ValueError("environment destination row out of range: a table writes WIND_N / WIND_E / WIND_D")
        acts: list[Action] = []
        rules, phases = [], []
        for p in range(len(self.names)):
            a0 = len(acts); acts += self._always[p]
            r0 = len(rules)
            for cond, ra, nxt in self._rules[p]:
                f = len(acts); acts += ra
                rules.append([cond.kind, cond.row, cond.cmp, cond.thr, cond.thr_par, f, len(ra), nxt])
            phases.append([a0, len(self._always[p]), r0, len(self._rules[p])])
        blob = [MAGIC, len(phases), len(rules), len(acts), self.n_par, self.n_rec, 0.0, 0.0]
        for ph in phases:
            blob += ph
        for r in rules:
            blob += r
        for a in acts:
            if a.dst == DST["REC"] and not 0 <= a.row < self.n_rec:
                raise ValueError("record row out of range")
            rowv = [a.dst, a.row, 1.0 if a.value.wrap else 0.0, a.value.c0, len(a.value.terms)]
            for k in range(NTERM):
                kind, row, c = a.value.terms[k] if k < len(a.value.terms) else (SRC["CONST"], 0, 0.0)
                if kind == SRC["PAR"] and not 0 <= row < self.n_par:
                    raise ValueError("parameter row out of range")
                rowv += [kind, row, c]
            assert len(rowv) == ACT_REC
            blob += rowv
        return np.asarray(blob, dtype=np.float64)


# ---- the same interpreter on the host, over arrays the caller supplies -------------------------------------------------------------
def _wrap(x):
    return x + 2 * np.pi * np.floor((np.pi - x) / (2 * np.pi))


def evaluate_on_host(blob: np.ndarray, st: dict, t: float, dt: float) -> None:
    """One evaluation of the table for every aircraft, in place. st: phase [n] int, since [n] int64 (step count at the entry of the phase),
    step (int: steps taken), par [n_par, n], rec [n_rec, n], cu, cs, u, ui, s (the model's arrays, modified in place; cu and cs only where the table
    names them — a Cessna172Sv0's dict has neither), and the outputs the
    sources name: on_gnd, h_e, psi, theta, phi, chi, EAS, clm [n]; x [rows, n] (device row order) where SRC X is used; active [n] bool
    (aircraft whose simulation has ended are not evaluated). The world's kinds: env [FB_NENV, n] (the rows of world.env) where the table names
    SRC / DST ENV — a wind row is written only where the value differs, and st["env_changed"] [n] bool is set (or OR-ed into) for those aircraft;
    y [FB_NY, n] (the output record at the state behind the step) where it names SRC Y — no action writes it, so it is the record as it stood when
    the evaluation began, also behind a wind write.
    The tapped outputs behind a wind write: on the device the `always` actions of a phase that read no tapped output run AHEAD of the evaluation of
    f_ode! the taps come from (stage A, then B: csrc/scenario_kernels.hpp), so a rule on EAS — the one tap that depends on the wind — sees the wind such
    an action has just written, while y_(FB_Y_AIR + 20) is the record's EAS from before it. The same order here: those `always` actions first, for every
    phase; then, if one of them changed a wind row and the caller gave st["retap"], retap(st) is called to renew the tapped entries of st under the new
    rows (host_callback: set_env, f_ode!, fetch); then the other `always` actions and the rules. Without `retap` the tapped entries stay as supplied."""
    assert blob[0] == MAGIC
    n_ph, n_rule, n_act = int(blob[1]), int(blob[2]), int(blob[3])
    PH = blob[HDR:HDR + PH_REC * n_ph].reshape(n_ph, PH_REC)
    RU = blob[HDR + PH_REC * n_ph:HDR + PH_REC * n_ph + RULE_REC * n_rule].reshape(n_rule, RULE_REC)
    AC = blob[HDR + PH_REC * n_ph + RULE_REC * n_rule:].reshape(n_act, ACT_REC)
    phase0 = st["phase"].copy()
    n = phase0.size

    def source(kind, row, m):
        kind, row = int(kind), int(row)
        if kind == SRC["CONST"]: return np.ones(m.sum())
        if kind == SRC["T"]: return np.full(m.sum(), t)
        if kind == SRC["T_IN_PHASE"]: return (st["step"] - st["since"][m]) * dt
        if kind == SRC["X"]: return st["x"][row, m]
        if kind == SRC["CS"]: return st["cs"][row, m]
        if kind == SRC["CU"]: return st["cu"][row, m]
        if kind == SRC["U"]: return st["u"][row, m]
        if kind == SRC["S"]: return st["s"][row, m].astype(np.float64)
        if kind == SRC["PAR"]: return st["par"][row, m]
        if kind == SRC["REC"]: return st["rec"][row, m]
        if kind == SRC["ENV"]: return st["env"][row, m]
        if kind == SRC["Y"]: return st["y"][row, m]
        name = {SRC["ON_GND"]: "on_gnd", SRC["H_E"]: "h_e", SRC["PSI"]: "psi", SRC["THETA"]: "theta", SRC["PHI"]: "phi", SRC["CHI"]: "chi",
                SRC["EAS"]: "EAS", SRC["CLM"]: "clm"}[kind]
        return np.asarray(st[name], dtype=np.float64)[m]

    def run(a, m):
        if not m.any():
            return
        v = np.full(m.sum(), a[3])
        for k in range(int(a[4])):
            kind, row, c = a[5 + 3 * k:8 + 3 * k]
            v = v + c * source(kind, row, m)
        if a[2] != 0:
            v = _wrap(v)
        dst, row = int(a[0]), int(a[1])
        if dst == DST["CU"]: st["cu"][row, m] = v
        elif dst == DST["U"]: st["u"][row, m] = v
        elif dst == DST["REC"]: st["rec"][row, m] = v
        elif dst == DST["ENV"]:
            differs = ~(st["env"][row, m] == v)   # (like the device: a wind row is written only where the value differs)
            idx = np.flatnonzero(m)[differs]
            st["env"][row, idx] = v[differs]
            st.setdefault("env_changed", np.zeros(n, bool))[idx] = True
        else:
            w = st["ui"][m]
            st["ui"][m] = np.where(v != 0, w | row, w & ~row)

    def taps(a):
        return any(int(a[5 + 3 * k]) in TAPPED and int(a[5 + 3 * k]) != SRC["H_E"] for k in range(int(a[4])))   # (H_E is a state row: scn_needs_y)

    ahead = [not any(taps(a) for a in AC[int(PH[p][0]):int(PH[p][0]) + int(PH[p][1])]) for p in range(n_ph)]
    changed0 = st["env_changed"].copy() if "env_changed" in st else np.zeros(n, bool)
    for p in range(n_ph):   # stage A of the device's walk: `always` actions that read no tapped output
        m = (phase0 == p) & st["active"]
        if ahead[p] and m.any():
            for a in AC[int(PH[p][0]):int(PH[p][0]) + int(PH[p][1])]:
                run(a, m)
    if "retap" in st and "env_changed" in st and (st["env_changed"] & ~changed0).any():
        st["retap"](st)
    for p in range(n_ph):
        m = (phase0 == p) & st["active"]
        if not m.any():
            continue
        a0, na, r0, nr = (int(v) for v in PH[p])
        if not ahead[p]:
            for a in AC[a0:a0 + na]:
                run(a, m)
        left = m.copy()
        for r in RU[r0:r0 + nr]:
            if not left.any():
                break
            lhs = np.zeros(n); lhs[left] = source(r[0], r[1], left)
            if r[4] >= 0:
                lhs = lhs - st["par"][int(r[4])]
            thr = np.full(n, r[3])
            c = int(r[2])
            hold = {CMP["<"]: lhs < thr, CMP[">"]: lhs > thr, CMP[">="]: lhs >= thr, CMP["<="]: lhs <= thr, CMP["=="]: lhs == thr, CMP["!="]: lhs != thr,
                    CMP["always"]: np.ones(n, bool)}[c] & left
            for a in AC[int(r[5]):int(r[5]) + int(r[6])]:
                run(a, hold)
            st["phase"][hold] = int(r[7])
            st["since"][hold] = st["step"]
            left &= ~hold


def table_kinds(blob: np.ndarray):
    """(source kinds, destination kinds) a packed table names"""
    n_ph, n_rule, n_act = int(blob[1]), int(blob[2]), int(blob[3])
    RU = blob[HDR + PH_REC * n_ph:HDR + PH_REC * n_ph + RULE_REC * n_rule].reshape(n_rule, RULE_REC)
    AC = blob[HDR + PH_REC * n_ph + RULE_REC * n_rule:].reshape(n_act, ACT_REC)
    srcs = {int(r[0]) for r in RU if int(r[2]) != CMP["always"]}
    for a in AC:
        srcs |= {int(a[5 + 3 * k]) for k in range(int(a[4]))}
    return srcs, {int(a[0]) for a in AC}


def host_callback(blob: np.ndarray, st: dict, dt: float, every: int = 1):
    """The table as the `user_callback` of a Simulation (the host-callback form of a run: every step crosses to the host). st: phase, since, par, rec
    as evaluate_on_host wants them; its `step` is counted here, and the table is evaluated behind every `every`-th step. Per evaluation the model's
    inputs (and a Cessna172Xv2's control-law rows) come down and go back; the outputs the table names are fetched after an f_ode! — the three blocks
    of the tapped outputs, or the whole record only for a table that names y_ — and the environment rows only for a table that names them, pushed
    back through set_env only when a wind row has changed. Where an `always` action has written the wind ahead of a tapped read, the taps are fetched
    again under the new rows (evaluate_on_host's `retap`), as the device's evaluation of f_ode! stands behind that write. Only the environment is
    pushed for that second f_ode!: on the device stage (B) also sees the u / ui / cu an `always` action has just written, but none of the eight taps
    (attitude, track, climb rate, EAS, weight on wheels) depends on them, so the bits agree; a tap that did would need those rows pushed here too."""
    from .modeling import f_ode
    srcs, dsts = table_kinds(blob)
    if SRC["X"] in srcs:
        raise ValueError("host_callback: x_ sources read the device's row order, which the host arrays do not have; evaluate such a table on the device")
    ctl = bool(srcs & {SRC["CS"], SRC["CU"]}) or DST["CU"] in dsts
    uses_env = SRC["ENV"] in srcs or DST["ENV"] in dsts
    kin, air, ldg = K["FB_Y_KIN"], K["FB_Y_AIR"], K["FB_Y_LDG"]
    st.setdefault("step", 0)

    def callback(mdl):
        st["step"] += 1
        if st["step"] % every:
            return
        u, ui = mdl.u, mdl.ui
        st.update(u=u, ui=ui, s=mdl.s, active=mdl.status == 0)
        if ctl:
            cu = mdl.cu
            st.update(cu=cu, cs=mdl.cs)
        if uses_env:
            st["env"] = mdl.env
            st["env_changed"] = np.zeros(mdl.n, bool)
        def fetch(whole):
            f_ode(mdl)
            if whole:
                y = st["y"] = mdl.y
                k_, a_, l_ = y[kin:], y[air:], y[ldg:]
            else:
                y = mdl.y_fields("KIN", "AIR", "LDG")
                k_, a_, l_ = y, y[air - kin:], y[air - kin + K["FB_Y_AERO"] - air:]
            st.update(h_e=k_[20], psi=k_[0], theta=k_[1], phi=k_[2], chi=k_[38], EAS=a_[20], clm=-k_[36],
                      on_gnd=((l_[1] + l_[12] + l_[23]) > 0).astype(np.float64))

        def retap(_):   # the taps under the wind an `always` action has just written (the record y stays the one from before)
            mdl.env = st["env"]
            fetch(False)
        if SRC["Y"] in srcs or srcs & set(TAPPED):
            fetch(SRC["Y"] in srcs)
            if srcs & set(TAPPED):
                st["retap"] = retap
        evaluate_on_host(blob, st, st["step"] * dt, dt)
        if ctl:
            mdl.cu = cu
        mdl.u = u
        mdl.ui = ui
        if uses_env and st["env_changed"].any():
            mdl.env = st["env"]
    return callback
