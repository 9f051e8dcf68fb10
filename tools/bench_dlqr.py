#!/usr/bin/env python3
"""Discrete LQR on the device: kernel times of k_lss_dlqr beside k_lqr (python3 tools/bench_dlqr.py [--systems N ...] [--out FILE]).

For (nx, nu) = (4, 1), (9, 8), (16, 4) at 4096 and 1 048 576 systems (the random systems of tests/lqr_prototype.py, 64 distinct ones tiled
over the batch — a kernel's time does not depend on where a system sits): fb_lss_dlqr on the world fb_lss_c2d makes at Ts = 0.02 with the
weights Ts Q, Ts R, and fb_lqr on the continuous source of the same plants with Q, R — the parent commit's kernel, unchanged, in the same
run. HIP events around the kernels from fb_timing_begin_per_launch, the median of 3 calls after one warm-up. Nothing is asserted; the
figures go to profiles/dlqr_bench.txt and docs/design/linearize.md."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
import lqr_prototype as proto  # noqa: E402

SHAPES = [(4, 1), (9, 8), (16, 4)]
SYSTEMS = [4096, 1 << 20]
TS = 0.02
DISTINCT = 64
_pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def stamps(w, calls, run):
    """the per-launch kernel times [ms] of `calls` runs on w's stream, after one warm-up"""
    run()
    check(fb.lib.fb_timing_begin_per_launch(w._h, calls))
    for _ in range(calls):
        run()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64)


def timed(w, Q, R, calls, discrete):
    """(kernel times [ms], iters, status, resid) of fb_lss_dlqr or fb_lqr on w: K, resid, iters and status come home, X does not"""
    n, nx, nu = w.n, w.nx, w.nu
    K, resid = np.empty(nu * nx * n), np.empty(n)
    iters, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    q, r = np.ascontiguousarray(Q.T).reshape(-1), np.ascontiguousarray(R.T).reshape(-1)
    if discrete:
        run = lambda: check(fb.lib.fb_lss_dlqr(w._h, _pd(q), _pd(r), _pd(K), None, _pd(resid), _pi(iters), _pi(status), None))
    else:
        run = lambda: check(fb.lib.fb_lqr(w._h, _pd(q), _pd(r), _pd(K), None, _pd(resid), _pi(iters), _pi(status)))
    return stamps(w, calls, run), iters, status, resid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--systems", type=int, nargs="+", default=SYSTEMS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_dlqr.py: Ts = {TS}, 1 warm-up + {a.calls} timed calls, medians; source hash {g.source_hash()}")
    results = []
    for nx, nu in SHAPES:
        A, B, Q, R = proto.systems(nx, nu, DISTINCT)
        for n in a.systems:
            reps = n // DISTINCT
            lss = fb.LinearizedSS(xdot0=np.zeros((n, nx)), x0=np.zeros((n, nx)), u0=np.zeros((n, nu)), y0=np.zeros((n, 1)),
                                  A=np.tile(A, (reps, 1, 1)), B=np.tile(B, (reps, 1, 1)), C=np.zeros((n, 1, nx)), D=np.zeros((n, 1, nu)),
                                  x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=tuple(f"u{k}" for k in range(nu)), y_labels=("y0",))
            w = fb.LinearWorld(lss)
            del lss
            ms_c, it_c, st_c, _ = timed(w, Q, R, a.calls, discrete=False)
            s = fb.c2d(w, TS)
            assert s.ok.all()
            ms_d, it_d, st_d, res_d = timed(s.world, TS * Q, TS * R, a.calls, discrete=True)
            s.world.close()
            w.close()
            m_c, m_d = float(np.median(ms_c)), float(np.median(ms_d))
            Pc, Pd = (8 if 2 * nx <= 8 else 16 if 2 * nx <= 16 else 32), (8 if nx <= 8 else 16)
            log(f"k_lqr      ({nx:2d}, {nu}) P={Pc:2d} systems {n:8d}: kernel median {m_c:9.3f} ms (min {ms_c.min():.3f}, max {ms_c.max():.3f}) | {n / (m_c * 1e-3):.3e} designs/s | "
                f"iterations {it_c.min()} / {int(np.median(it_c))} / {it_c.max()} | status != 0: {int((st_c != 0).sum())}")
            log(f"k_lss_dlqr ({nx:2d}, {nu}) P={Pd:2d} systems {n:8d}: kernel median {m_d:9.3f} ms (min {ms_d.min():.3f}, max {ms_d.max():.3f}) | {n / (m_d * 1e-3):.3e} designs/s | "
                f"doublings {it_d.min()} / {int(np.median(it_d))} / {it_d.max()} | status != 0: {int((st_d != 0).sum())} | resid <= {np.nanmax(res_d):.2e} | "
                f"{m_d / m_c:.3f} of k_lqr")
            results.append(dict(nx=nx, nu=nu, systems=n, lqr_ms=[round(float(v), 4) for v in ms_c], dlqr_ms=[round(float(v), 4) for v in ms_d], ratio=m_d / m_c))
    log(json.dumps({"bench_dlqr": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
