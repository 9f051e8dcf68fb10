#!/usr/bin/env python3
"""Milliseconds per evaluation of a scenario table for N aircraft (default 1 048 576): the tables that reach the world (FB_SCN_DST_ENV, FB_SCN_SRC_Y)
beside the Cessna172Xv2 landing table of examples/crosswind_landing.py, same method as tools/bench_scenario_sv0.py (HIP events around `steps`
one-step launches with the table evaluated after every step and with the scenario off; the difference per step; median / min / max over `windows`
pairs): python3 tools/bench_scenario_world.py [n] [steps] [windows]. With FLIGHTBATCH_LIB pointing at a library that lacks the world kinds, those
tables are reported as refused and the landing table alone is timed (the A/B against a parent build)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "flight.jl_amd"), os.path.join(ROOT, "examples")]
import flightbatch as fb  # noqa: E402
from flightbatch import scenario as sc  # noqa: E402


def window(w, steps):
    ms, launches = C.c_float(), C.c_int64()
    fb._lib.check(fb.lib.fb_timing_begin(w._h))
    fb._lib.check(fb.lib.fb_step(w._h, steps))
    fb._lib.check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(launches)))
    return float(ms.value)


def wind_table():
    """one `always` wind action: WIND_E = par(0) + 0.01 T — a new value, one row write and one invalidation per aircraft and evaluation"""
    scn = sc.Scenario(n_par=1, n_rec=1)
    scn.always(scn.phase("gusty"), [sc.env("WIND_E", sc.par(0) + 0.01 * sc.src.T)])
    return scn


def y_table():
    """one rule on an output row (TAS below a threshold that never comes): fb_step refreshes the whole record ahead of every evaluation"""
    scn = sc.Scenario(n_par=1, n_rec=1)
    wait, done = scn.phase("wait"), scn.phase("done")
    scn.when(wait, sc.y_(fb.K["FB_Y_AIR"] + 19) - sc.par(0) < 0.0, [sc.rec(0, sc.src.T)], then=done)
    return scn


def per_evaluation(w, load, steps, windows):
    out = []
    for k in range(windows + 1):   # (the first pair warms up)
        load()
        on = window(w, steps)
        w.set_scenario(None)
        off = window(w, steps)
        if k:
            out.append((on - off) / steps)
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), step_ms=off / steps)


def trimmed(make, n):
    w = make()
    w.set_env()
    fb.f_init(w, fb.TrimParameters(EAS=np.linspace(38.0, 52.0, n), h_e=np.linspace(500.0, 2500.0, n)))
    assert w.trim_success.all()
    fb.Simulation(w, dt=0.02, save_on=False, steps_per_launch=1)
    return w


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    res = {"n": n, "steps_per_window": steps, "windows": windows, "library": os.path.basename(fb._lib.LIB_PATH)}
    import crosswind_landing
    far = np.zeros((12, n)); far[3] = 1e-3          # the landing table's end-point rows (any segment: the aircraft stay on the final leg, 500 m and more above the row-7 altitude)
    x2 = trimmed(lambda: fb.Cessna172Xv2World(n), n)
    landing = crosswind_landing.scenario_table(True)
    res["Cessna172Xv2 landing table"] = per_evaluation(x2, lambda: x2.set_scenario(landing, params=far[:9], every=1), steps, windows)
    assert (x2.status == 0).all()
    x2.close()
    for model, make in (("Cessna172Xv2", lambda: fb.Cessna172Xv2World(n)), ("Cessna172Sv0", lambda: fb.BatchedWorld(n))):
        w = trimmed(make, n)   # (a fresh batch in trimmed flight: the landing table's aircraft have flown towards its segment)
        for name, scn, par in (("one always wind action", wind_table(), np.zeros((1, n))), ("one rule on an output row", y_table(), np.full((1, n), -1e9))):
            try:
                res[f"{model} {name}"] = per_evaluation(w, lambda: w.set_scenario(scn, params=par, every=1), steps, windows)
            except fb.FlightBatchError as e:
                res[f"{model} {name}"] = {"refused": str(e)[:80]}
        assert (w.status == 0).all()
        w.close()
    for k, r in res.items():
        if isinstance(r, dict) and "median_ms" in r:
            print(f"{k:45s} {r['median_ms']:.4f} ms per evaluation of {n} aircraft (min {r['min_ms']:.4f}, max {r['max_ms']:.4f}); a one-step launch without the table: {r['step_ms']:.3f} ms")
    print(json.dumps(res))
