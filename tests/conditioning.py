"""A MEASURED conditioning bound for aircraft that roll on their wheels (test infrastructure).

Two things make a long ground roll ill-conditioned. (1) The reference computes a strut's compression as a difference of ECEF positions
(FlightPhysics/src/landinggear.jl:240-275: wheel and terrain point, both 6.4e6 m from the Earth's centre), so the contact geometry
resolves 2^-30 m = 9.3e-10 m — one ulp of the geocentric radius — and any two correct evaluations that round in a different order
(this library's second-order expansion about the body origin against the reference's two conversions) differ by that much at EVERY
evaluation, in front of 4e4 N/m of strut stiffness. (2) The friction regulators (landinggear.jl:411-476: PI compensators with
k_i = 400 1/s behind a sign-tested anti-windup halt, integrated by RK4 at dt = 0.01) amplify such differences along the roll, and now and
then a regulator halts one step apart in two runs, which carry that difference from there on.

How much, on the very aircraft of a test, is measured here instead of asserted in a comment: the CPU oracle is run again, K times, with
    * the body velocity v_eb_b of every aircraft nudged ONCE, as it comes within reach of the runway, by `rel` = 1e-12 — the size of the
      GPU's own distance from the oracle after an airborne approach (tests/test_gpu_c172x.py: closed loop 1e-11 after 1000 steps) —
    * and its altitude h_e moved by +/- one ulp of the geocentric radius (`jitter` = 9.3e-10 m, random sign) at every step while it is
      within reach of the runway: the resolution of the contact geometry, (1) above.
(`rel=None, jitter=0` gives the one-ulp-at-touchdown experiment whose numbers the test log quotes as well.) |oracle - oracle'| per
aircraft is the ENVELOPE; the GPU is then held to

    per aircraft     |gpu - oracle| <= max(1e-6, 10 x envelope)      — so an aircraft whose envelope is below 1e-7 holds the 1e-6 of the
                     north star — for all but as many aircraft as ONE ORACLE RUN leaves outside the envelope of the other K - 1
                     (a regulator that halts a step apart is a rare, discrete event that no other sample predicts: the count is
                     measured the same way for the oracle against itself, leave-one-out);
    distribution     the 50 / 90 / 99 % quantiles and the maximum of the GPU's per-aircraft errors within 10 x those of the pooled
                     oracle-vs-oracle' errors (floor 1e-6).

No hand-set tolerance is left: every number on the right-hand side comes from the oracle, run on the same inputs."""
import numpy as np


def nudge(v, rel, sign):
    """v moved by one ulp (rel None) or by the relative amount rel, in the direction sign (+1 / -1 per entry)"""
    if rel is None:
        return np.nextafter(v, np.where(sign > 0, np.inf, -np.inf))
    return v * (1.0 + rel * sign)


ULP_R = float(np.spacing(6.4e6))   # 2^-30 m: one ulp of the geocentric radius


def x2_perturbed_runs(X, start, env, nsteps, h_row, h_runway, rel, K=4, jitter=0.0, chunk=10, reach=8.0, seed=0, threads=0, ratio=2):
    """K oracle runs of Cessna172Xv2 (OracleX dict `start`: x in ORACLE row order, u, ui, s, cu, cs) over nsteps steps at dt = 0.01,
    Δt = ratio x 0.01, each with v_eb_b (oracle rows 24-26) nudged once per aircraft, at the first chunk boundary at which its altitude row is
    within `reach` metres of the runway, and — jitter > 0 — its altitude moved by +/- jitter at every step from there on. Returns the
    list of final dicts."""
    rng = np.random.default_rng(seed)
    n = start["x"].shape[1]
    if jitter > 0:
        chunk = 1
    outs = []
    for k in range(K):
        o = {key: np.array(val, copy=True) for key, val in start.items() if isinstance(val, np.ndarray)}
        o["status"] = np.zeros(n, np.int32); o["nstep"] = 0
        o.pop("term_step", None); o.pop("term_where", None)
        done = np.zeros(n, bool)
        sign = rng.choice([-1.0, 1.0], (3, n))
        left = nsteps
        while left > 0:
            near = (o["x"][h_row] - h_runway < reach) & (o["status"] == 0)
            now = near & ~done
            if now.any():
                o["x"][24:27, now] = nudge(o["x"][24:27, now], rel, sign[:, now])
                done |= now
            if jitter > 0 and near.any():
                o["x"][h_row, near] += jitter * rng.choice([-1.0, 1.0], int(near.sum()))
            m = min(chunk, left)
            X.step_term(o, env, 0.01, ratio, m, threads=threads)
            left -= m
        o["nudged"] = done
        outs.append(o)
    return outs


def s0_perturbed_runs(oracle, x0, u, ui, s0, env, nsteps, h_runway, rel, K=4, jitter=0.0, chunk=10, reach=8.0, seed=0, threads=0):
    """the same for Cessna172Sv0 (27-row oracle order, WA: altitude row 20): list of (x, s, status)"""
    rng = np.random.default_rng(seed)
    n = x0.shape[1]
    if jitter > 0:
        chunk = 1
    outs = []
    for k in range(K):
        x = np.array(x0, copy=True); s = np.array(s0, copy=True); st = np.zeros(n, np.int32)
        done = np.zeros(n, bool)
        sign = rng.choice([-1.0, 1.0], (3, n))
        left, step0 = nsteps, 0
        while left > 0:
            near = (x[20] - h_runway < reach) & (st == 0)
            now = near & ~done
            if now.any():
                x[24:27, now] = nudge(x[24:27, now], rel, sign[:, now])
                done |= now
            if jitter > 0 and near.any():
                x[20, near] += jitter * rng.choice([-1.0, 1.0], int(near.sum()))
            m = min(chunk, left)
            x, s, st, _, _ = oracle.step_term(x, u, ui, s, env, 0.01, m, step0=step0, status=st, threads=threads)
            left -= m; step0 += m
        outs.append((x, s, st))
    return outs


def check_against_envelope(err_gpu, E, label, floor=1e-6, factor=10.0):
    """err_gpu [lanes]: per-aircraft max scaled |gpu − oracle|; E [K x lanes]: per-aircraft max scaled |oracle_k′ − oracle|.
    Prints the measured numbers and asserts the bound of the module docstring."""
    err_gpu = np.asarray(err_gpu); E = np.asarray(E)
    K = E.shape[0]
    env = E.max(0)
    q = [0.5, 0.9, 0.99, 1.0]
    qg, qe = np.quantile(err_gpu, q), np.quantile(E.ravel(), q)
    print(f"{label}: per-aircraft error quantiles 50/90/99/100 %: gpu vs oracle {qg}; oracle vs oracle' (pooled over {K} runs) {qe}")
    outside = err_gpu > np.maximum(floor, factor * env)
    loo = []
    for k in range(K):
        others = np.delete(E, k, axis=0).max(0)
        loo.append(int((E[k] > np.maximum(floor, factor * others)).sum()))
    well = env < floor / factor
    print(f"{label}: {int(well.sum())} of {err_gpu.size} aircraft have an envelope below {floor / factor:.0e} "
          f"(gpu max among them {err_gpu[well].max() if well.any() else 0.0:.2e}); outside max({floor:.0e}, {factor:g} x envelope): gpu {int(outside.sum())}, "
          f"one oracle run against the other {K - 1}: {loo}")
    assert outside.sum() <= max(loo) + 1, (label, int(outside.sum()), loo, np.flatnonzero(outside)[:8], err_gpu[outside][:8], env[outside][:8])
    for a, b, name in zip(qg, qe, ("median", "90 %", "99 %", "max")):
        assert a <= max(floor, factor * b), (label, name, a, b)
    return env
