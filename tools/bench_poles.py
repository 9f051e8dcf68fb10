#!/usr/bin/env python3
"""Poles on the device: kernel times of k_poles (python3 tools/bench_poles.py [--small] [--out FILE]).

fb_lss_poles at N = 1 048 576 for nx = 4, 9, 16, 32: the random systems of tests/poles_prototype.py (4096 distinct ones, tiled over the
batch — the kernel's time does not depend on where a system sits, but a wave waits for its slowest group, so the tiling keeps the mix of
neighbours the tests have), HIP events around the kernel from fb_timing_begin_per_launch, one warm-up call. Beside it the way the project
got these numbers before: np.linalg.eigvals in a host loop, timed on 256 of the same systems and scaled to the batch (the 2 KB per system
that would have to come home first are not in that figure)."""
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
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
import poles_prototype as proto  # noqa: E402

SIZES = [4, 9, 16, 32]
DISTINCT = 4096
_pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def timed_poles(w, calls):
    n, nx = w.n, w.nx
    re, im = np.empty(nx * n), np.empty(nx * n)
    iters, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    run = lambda: check(fb.lib.fb_lss_poles(w._h, _pd(re), _pd(im), _pi(iters), _pi(status)))
    run()                                                   # warm-up
    check(fb.lib.fb_timing_begin_per_launch(w._h, calls))
    for _ in range(calls):
        run()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64), iters, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1/16 of the batch (a quick look)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES, help="the nx to time (default 4 9 16 32; nx = 32 takes 8 GB of host memory per copy of A)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = (1 << 20) // (16 if a.small else 1)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_poles.py{' --small' if a.small else ''}: N = {n}, 1 warm-up + {a.calls} timed calls of fb_lss_poles; source hash {g.source_hash()}")
    results = []
    for nx in a.sizes:
        A = proto.systems(nx, DISTINCT)
        reps = n // DISTINCT
        lss = fb.LinearizedSS(xdot0=np.zeros((n, nx)), x0=np.zeros((n, nx)), u0=np.zeros((n, 1)), y0=np.zeros((n, 1)),
                              A=np.tile(A, (reps, 1, 1)), B=np.zeros((n, nx, 1)), C=np.zeros((n, 1, nx)), D=np.zeros((n, 1, 1)),
                              x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=("u0",), y_labels=("y0",))
        w = fb.LinearWorld(lss)
        del lss
        ms, iters, status = timed_poles(w, a.calls)
        w.close()
        P = proto.group(nx)
        rate = n / (np.median(ms) * 1e-3)
        t0 = time.perf_counter()
        for i in range(256):
            np.linalg.eigvals(A[i])
        t_host = (time.perf_counter() - t0) / 256
        log(f"nx {nx:2d} P={P:2d}: kernel median {np.median(ms):9.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | {rate:.3e} systems/s | "
            f"sweeps min {iters.min()} / median {int(np.median(iters))} / max {iters.max()} | status != 0: {int((status != 0).sum())} | "
            f"np.linalg.eigvals host loop {t_host * 1e6:.0f} us per system (256 timed) = {t_host * n:.1f} s for the batch, "
            f"{t_host * n / (np.median(ms) * 1e-3):.0f} x the kernel")
        results.append(dict(nx=nx, P=P, n=n, ms=[round(float(v), 4) for v in ms], systems_per_s=rate,
                            sweeps=[int(iters.min()), int(np.median(iters)), int(iters.max())], eigvals_s_per_system=t_host))
    log(json.dumps({"bench_poles": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
