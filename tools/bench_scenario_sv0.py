#!/usr/bin/env python3
"""Milliseconds per evaluation of a scenario table for N aircraft (default 1 048 576), Cessna172Sv0 (k_scenario_sv0) beside the yardstick, the
Cessna172Xv2 instance (k_scenario), in the same process on the same device: python3 tools/bench_scenario_sv0.py [n] [steps] [windows].

Two tables, valid on both models: a MEMORY-ONLY one (every aircraft waits for `T - par(0) >= 0` with a time that never comes: the walk reads the
clock and a parameter row, no wave evaluates f_ode!) and one where EVERY WAVE needs vehicle.y (every aircraft waits for `THETA - par(0) > 0` with an
angle that never comes: one ground-capable evaluation of f_ode! with the partial sink per aircraft and evaluation).

Method: HIP events on the handle's stream (fb_timing_begin / fb_timing_end) around `steps` one-step launches, once with the table evaluated after
every step and once with the scenario switched off; the difference, divided by `steps`, is the time the evaluation adds to a step (the kernel plus
whatever its launch costs the queue). Median, minimum and maximum over `windows` pairs of windows; one JSON line at the end."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flight.jl_amd"))
import flightbatch as fb  # noqa: E402
from flightbatch import scenario as sc  # noqa: E402


def table(reads_y: bool):
    scn = sc.Scenario(n_par=1, n_rec=1)
    wait, done = scn.phase("wait"), scn.phase("done")
    cond = (sc.src.THETA - sc.par(0) > 0.0) if reads_y else (sc.src.T - sc.par(0) >= 0.0)
    scn.when(wait, cond, [sc.rec(0, sc.src.T)], then=done)
    return scn


def window(w, steps):
    ms, launches = C.c_float(), C.c_int64()
    fb._lib.check(fb.lib.fb_timing_begin(w._h))
    fb._lib.check(fb.lib.fb_step(w._h, steps))
    fb._lib.check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(launches)))
    assert launches.value == steps, (launches.value, steps)
    return float(ms.value)


def measure(make_world, n, steps, windows):
    w = make_world()
    fb.f_init(w, fb.TrimParameters(EAS=np.linspace(38.0, 52.0, n), h_e=np.linspace(500.0, 2500.0, n)))
    assert w.trim_success.all()
    fb.Simulation(w, dt=0.02, save_on=False, steps_per_launch=1)
    out = {}
    for name, reads_y in (("memory_only", False), ("every_wave_reads_y", True)):
        per_eval = []
        for k in range(windows + 1):   # (the first pair warms up)
            w.set_scenario(table(reads_y), params=np.full((1, n), 1e9), every=1)
            on = window(w, steps)
            assert (w.scenario_state()["phase"] == 0).all()
            w.set_scenario(None)
            off = window(w, steps)
            if k:
                per_eval.append((on - off) / steps)
        out[name] = dict(median_ms=float(np.median(per_eval)), min_ms=float(min(per_eval)), max_ms=float(max(per_eval)), step_ms=off / steps)
    assert (w.status == 0).all()
    w.close()
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    res = {"n": n, "steps_per_window": steps, "windows": windows,
           "Cessna172Sv0": measure(lambda: fb.BatchedWorld(n), n, steps, windows),
           "Cessna172Xv2": measure(lambda: fb.Cessna172Xv2World(n), n, steps, windows)}
    for model in ("Cessna172Sv0", "Cessna172Xv2"):
        for name, r in res[model].items():
            print(f"{model:13s} {name:20s} {r['median_ms']:.4f} ms per evaluation of {n} aircraft (min {r['min_ms']:.4f}, max {r['max_ms']:.4f}); "
                  f"a one-step launch without the table: {r['step_ms']:.3f} ms")
    print(json.dumps(res))
