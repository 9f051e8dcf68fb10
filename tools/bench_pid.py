#!/usr/bin/env python3
"""PID loop design on the device: kernel times of fb_pid_metrics (python3 tools/bench_pid.py [--out FILE]).

One call = k_lss_freqresp (P(jw) of every system on the grid) then k_pid_metrics (every (system, candidate) pair), each between its own pair
of HIP events (fb_timing_begin_per_launch). Plants: the random passive nx = 9 systems of tests/pid_prototype.py (the q2e plant's size),
t_sim = 10, dt = 2e-3 (5000 RK4 steps), 321 frequencies, 12 candidates per system: the shape of one poll of optimize_pid on the reference's
q2e design. Batches: the reference's 28 nodes, and 4096 systems. Nothing gates on these numbers."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
import pid_prototype as proto  # noqa: E402

NX, M, T_SIM, DT = 9, 12, 10.0, 2e-3
DISTINCT = 256


def timed(w, pts, calls):
    """per-launch times [calls, 2] in ms (frequency response, metrics) of `calls` fb_pid_metrics calls after one warm-up"""
    st = fb.Settings(t_sim=T_SIM, dt=DT, w=proto.Q2E_GRID)
    run = lambda: fb.pid_metrics(w, pts, settings=st, weights=proto.Q2E_WEIGHTS)
    res = run()
    check(fb.lib.fb_timing_begin_per_launch(w._h, 2 * calls))
    for _ in range(calls):
        run()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64).reshape(calls, 2), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--large", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_pid.py: nx = {NX}, {M} candidates per system, {int(round(T_SIM / DT))} RK4 steps, {proto.Q2E_GRID.size} frequencies; "
        f"1 warm-up + {a.calls} timed calls of fb_pid_metrics; source hash {g.source_hash()}")
    A, b, c, d = proto.plants(NX, DISTINCT)
    P = proto.points(DISTINCT, M)
    results = []
    for n in (28, a.large):
        idx = np.arange(n) % DISTINCT
        w = fb.LinearWorld(proto.model(fb, A[idx], b[idx], c[idx], d[idx]))
        ms, res = timed(w, P[idx], a.calls)
        w.close()
        fr, mt = np.median(ms[:, 0]), np.median(ms[:, 1])
        log(f"N = {n:5d} x m = {M}: k_lss_freqresp median {fr:8.3f} ms (min {ms[:, 0].min():.3f}, max {ms[:, 0].max():.3f}) | k_pid_metrics median {mt:8.3f} ms "
            f"(min {ms[:, 1].min():.3f}, max {ms[:, 1].max():.3f}) | {n * M / (mt * 1e-3):.3e} pairs/s | the frequency response costs "
            f"{fr / (mt / M):.2f} candidates per system | status != 0: {int((res.status != 0).sum())}")
        results.append(dict(n=n, m=M, freqresp_ms=[round(float(v), 4) for v in ms[:, 0]], metrics_ms=[round(float(v), 4) for v in ms[:, 1]]))
    log(json.dumps({"bench_pid": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
