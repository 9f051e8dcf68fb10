#!/usr/bin/env python3
"""LQR design on the device: kernel times of k_lqr (python3 tools/bench_lqr.py [--small] [--out FILE]).

fb_lqr at N = 1 048 576 for (nx, nu) = (8, 2), (11, 2), (16, 4): the random systems of tests/lqr_prototype.py (4096 distinct ones, tiled over
the batch — the kernel's time does not depend on where a system sits), HIP events around the kernel from fb_timing_begin_per_launch, one
warm-up call. Beside it the only other way to the same gains: scipy's solve_continuous_are in a host loop, timed on 256 of the same systems
and scaled to the batch."""
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
import lqr_prototype as proto  # noqa: E402

SHAPES = [(8, 2), (11, 2), (16, 4)]
DISTINCT = 4096
_pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def timed_design(w, Q, R, calls):
    n, nx, nu = w.n, w.nx, w.nu
    K, resid = np.empty(nu * nx * n), np.empty(n)
    iters, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    q, r = np.ascontiguousarray(Q.T).reshape(-1), np.ascontiguousarray(R.T).reshape(-1)
    run = lambda: check(fb.lib.fb_lqr(w._h, _pd(q), _pd(r), _pd(K), None, _pd(resid), _pi(iters), _pi(status)))
    run()                                                   # warm-up
    check(fb.lib.fb_timing_begin_per_launch(w._h, calls))
    for _ in range(calls):
        run()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64), iters, status, resid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1/16 of the batch (a quick look)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = (1 << 20) // (16 if a.small else 1)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_lqr.py{' --small' if a.small else ''}: N = {n}, 1 warm-up + {a.calls} timed calls of fb_lqr; source hash {g.source_hash()}")
    results = []
    for nx, nu in SHAPES:
        A, B, Q, R = proto.systems(nx, nu, DISTINCT)
        reps = n // DISTINCT
        lss = fb.LinearizedSS(xdot0=np.zeros((n, nx)), x0=np.zeros((n, nx)), u0=np.zeros((n, nu)), y0=np.zeros((n, 1)),
                              A=np.tile(A, (reps, 1, 1)), B=np.tile(B, (reps, 1, 1)), C=np.zeros((n, 1, nx)), D=np.zeros((n, 1, nu)),
                              x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=tuple(f"u{k}" for k in range(nu)), y_labels=("y0",))
        w = fb.LinearWorld(lss)
        del lss
        ms, iters, status, resid = timed_design(w, Q, R, a.calls)
        w.close()
        P = 8 if 2 * nx <= 8 else 16 if 2 * nx <= 16 else 32
        rate = n / (np.median(ms) * 1e-3)
        t0 = time.perf_counter()
        for i in range(256):
            proto.scipy_lqr(A[i], B[i], Q, R)
        t_host = (time.perf_counter() - t0) / 256
        log(f"({nx:2d}, {nu}) P={P:2d}: kernel median {np.median(ms):9.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | {rate:.3e} designs/s | "
            f"iterations min {iters.min()} / median {int(np.median(iters))} / max {iters.max()} | status != 0: {int((status != 0).sum())} | "
            f"resid <= {np.nanmax(resid):.2e} | scipy host loop {t_host * 1e6:.0f} us per design (256 timed) = {t_host * n:.1f} s for the batch, "
            f"{t_host * n / (np.median(ms) * 1e-3):.0f} x the kernel")
        results.append(dict(nx=nx, nu=nu, P=P, n=n, ms=[round(float(v), 4) for v in ms], designs_per_s=rate,
                            iters=[int(iters.min()), int(np.median(iters)), int(iters.max())], scipy_s_per_design=t_host))
    log(json.dumps({"bench_lqr": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
