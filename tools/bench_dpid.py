#!/usr/bin/env python3
"""Discrete PID design on the device: k_dpid_metrics against k_pid_metrics (python3 tools/bench_dpid.py [--systems N ...] [--out FILE]).

Both kernels evaluate one candidate per system on the same plants at the same number of samples: k_pid_metrics integrates the continuous
loop by RK4 (four broadcast exchanges per sample), k_dpid_metrics steps the zero-order hold of the same plants under the sampled law (one
exchange per tick). Plants: the random passive systems of tests/pid_prototype.py, 256 distinct ones tiled over batches of 4096 and 2^20
systems, nx = 4, 9 and 20 (lane groups of 8, 16 and 32 on both sides); 4096 samples, seven frequencies (the grid pass is not what is compared). Both sides run in one process, alternating after a warm-up call each; every launch sits between its own pair of HIP events
(fb_timing_begin_per_launch), and the time quoted is the metrics kernel's alone. Nothing gates on these numbers."""
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

N_SAMPLES, TS, DT, DISTINCT = 4096, 0.02, 1e-3, 256


def stamps(w):
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--systems", type=int, nargs="*", default=[4096, 1 << 20])
    ap.add_argument("--nx", type=int, nargs="*", default=[4, 9, 20])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    import __graft_entry__ as g
    grid = np.logspace(-1.0, 2.0, 7)
    log(f"# tools/bench_dpid.py: one candidate per system, {N_SAMPLES} samples (RK4 steps at dt = {DT} | ticks at Ts = {TS}), {grid.size} frequencies; "
        f"1 warm-up + {a.calls} timed calls a side, alternating; source hash {g.source_hash()}")
    results = []
    for n, nx in ((n, nx) for n in a.systems for nx in a.nx):
        A, b, c, d = proto.plants(nx, DISTINCT)
        P = proto.points(DISTINCT, 1)
        idx = np.arange(n) % DISTINCT
        wc = fb.LinearWorld(proto.model(fb, A[idx], b[idx], c[idx], d[idx]))
        wd = fb.c2d(wc, TS).world
        pts = P[idx]
        cont = lambda: fb.pid_metrics(wc, pts, settings=fb.Settings(t_sim=N_SAMPLES * DT, dt=DT, w=grid))
        disc = lambda: fb.dpid_metrics(wd, pts, settings=fb.Settings(t_sim=N_SAMPLES * TS), w=grid)
        rc, rd = cont(), disc()
        check(fb.lib.fb_timing_begin_per_launch(wc._h, 2 * a.calls))
        check(fb.lib.fb_timing_begin_per_launch(wd._h, 2 * a.calls))
        for _ in range(a.calls):
            cont()
            disc()
        tc, td = stamps(wc).reshape(a.calls, 2)[:, 1], stamps(wd).reshape(a.calls, 2)[:, 1]
        wc.close()
        wd.close()
        mc, md = float(np.median(tc)), float(np.median(td))
        log(f"N = {n:7d}, nx = {nx:2d}: k_pid_metrics median {mc:9.3f} ms (min {tc.min():.3f}, max {tc.max():.3f}) | k_dpid_metrics median {md:9.3f} ms "
            f"(min {td.min():.3f}, max {td.max():.3f}) | ratio {mc / md:.2f} | {n * N_SAMPLES / (md * 1e-3):.3e} pair-ticks/s | "
            f"status != 0: {int((rc.status != 0).sum())}, {int((rd.status != 0).sum())}")
        results.append(dict(nx=nx, systems=n, samples=N_SAMPLES, pid_ms=[round(float(v), 4) for v in tc], dpid_ms=[round(float(v), 4) for v in td]))
    log(json.dumps({"bench_dpid": results}))


if __name__ == "__main__":
    main()
