#!/usr/bin/env python3
"""Margins on the device: kernel times of fb_lss_margins (python3 tools/bench_margins.py [--out FILE]).

One call = k_lss_freqresp (stage 1: L on the grid, the parent's kernel, timed here in the same run as the reference of the ratio) then
k_lss_margins (stage 2: brackets, bisection, selection), each between its own pair of HIP events (fb_timing_begin_per_launch); the median
of 3 calls after a warm-up. Plants: K / (s + 1)³ with K = 2, 4, 7 among nx = 4, 9, 20 states behind a random orthogonal change of state
(tests/margins_prototype.py: one phase and one gain crossing each, so about 2 x 48 eliminations of refinement beside the grid's 321), 64
distinct ones tiled over 4096 and 1 048 576 systems, on pidopt.default_grid(). The numpy prototype is timed on a few systems in a host loop,
for scale. Nothing gates on these numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
import margins_prototype as proto  # noqa: E402

NX_ALL, SYSTEMS, DISTINCT, CALLS, HOST_SYSTEMS = (4, 9, 20), (4096, 1 << 20), 64, 3, 4


def timed(w, grid, calls):
    """per-call times [calls, 2] in ms (grid response: the sum over its slices; margins) of `calls` fb_lss_margins calls after one
    warm-up, and the number of slices"""
    run = lambda: fb.margins(w, w=grid)
    res = run()
    check(fb.lib.fb_timing_begin_per_launch(w._h, 64 * calls))
    for _ in range(calls):
        run()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    ms = np.array(buf[:nl.value], dtype=np.float64).reshape(calls, -1)
    return np.stack([ms[:, :-1].sum(axis=1), ms[:, -1]], axis=1), res, ms.shape[1] - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=CALLS)
    ap.add_argument("--systems", type=int, nargs="*", default=list(SYSTEMS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    grid = fb.pidopt.default_grid()
    log(f"# tools/bench_margins.py: K / (s + 1)^3 among nx states, {DISTINCT} distinct systems tiled, {grid.size} frequencies; 1 warm-up + "
        f"{a.calls} timed calls of fb_lss_margins; source hash {g.source_hash()}")
    results = []
    for nx in NX_ALL:
        rng = np.random.default_rng(nx)
        systems = [proto.embed(proto.cube(proto.K_CLOSED[k % 3]), nx, rng) for k in range(DISTINCT)]
        t0 = time.perf_counter()
        for s in systems[:HOST_SYSTEMS]:
            proto.margins(*s, grid)
        host = (time.perf_counter() - t0) / HOST_SYSTEMS
        M = proto.lss_arrays(systems, nu=1, ny=1, iu=0, iy=0)
        for n in a.systems:
            reps = n // DISTINCT
            tile = lambda m: np.tile(m, (reps,) + (1,) * (m.ndim - 1))
            w = fb.LinearWorld(fb.LinearizedSS(**{k: tile(v) for k, v in M.items()}, x_labels=tuple(f"x{k}" for k in range(nx)),
                                               u_labels=("u",), y_labels=("y",)))
            ms, res, slices = timed(w, grid, a.calls)
            w.close()
            s1, s2 = float(np.median(ms[:, 0])), float(np.median(ms[:, 1]))
            log(f"nx = {nx:2d}, N = {n:7d}: k_lss_freqresp ({slices} launch{'es' if slices > 1 else ''}) median {s1:9.3f} ms (min {ms[:, 0].min():.3f}, max {ms[:, 0].max():.3f}) | k_lss_margins median "
                f"{s2:9.3f} ms (min {ms[:, 1].min():.3f}, max {ms[:, 1].max():.3f}) | stage 2 / stage 1 = {s2 / s1:.3f} | {n / ((s1 + s2) * 1e-3):.3e} systems/s | "
                f"crossings per system {float((res.npc + res.ngc).mean()):.2f}, status != 0: {int((res.status != 0).sum())} | the numpy prototype: "
                f"{host * 1e3:.1f} ms per system in a host loop")
            results.append(dict(nx=nx, n=n, slices=slices, freqresp_ms=[round(float(v), 4) for v in ms[:, 0]], margins_ms=[round(float(v), 4) for v in ms[:, 1]],
                                prototype_ms_per_system=round(host * 1e3, 3)))
    log(json.dumps({"bench_margins": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
