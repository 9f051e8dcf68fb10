#!/usr/bin/env python3
"""Step responses on the device: kernel times of k_timeresp (python3 tools/bench_stepinfo.py [--pairs N ...] [--out FILE]).

fb_lss_stepinfo (info only, no sample buffer) over 5000 RK4 steps per pass at 4096 and 1 048 576 (system, channel) pairs for nx = 4, 9, 20:
the random stable plants of tests/timeresp_prototype.py (64 distinct ones, tiled over the batch, one channel), HIP events around the kernel
from fb_timing_begin_per_launch, the median of 3 calls after one warm-up. Beside it the way the project answered the question before: the
numpy prototype's RK4 loop and its StepInfo on the host, timed on the 64 distinct systems and scaled to the batch (the matrices that would
have to come home first are not in that figure)."""
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
import timeresp_prototype as proto  # noqa: E402

SIZES = [4, 9, 20]
PAIRS = [4096, 1 << 20]
STEPS, DT = 5000, 1e-3
DISTINCT = 64
_pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def timed_stepinfo(w, calls):
    n = w.n
    ch = np.zeros(1, dtype=np.int32)
    info, status = np.empty((9, 1, n)), np.empty((1, n), dtype=np.int32)
    run = lambda: check(fb.lib.fb_lss_stepinfo(w._h, _pi(ch), _pi(ch), 1, STEPS * DT, DT, None, None, None, 1, None, _pd(info), _pi(status)))
    run()                                                   # warm-up
    check(fb.lib.fb_timing_begin_per_launch(w._h, calls))
    for _ in range(calls):
        run()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64), info, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--pairs", type=int, nargs="+", default=PAIRS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_stepinfo.py: {STEPS} steps per pass, two passes, 1 warm-up + {a.calls} timed calls of fb_lss_stepinfo; source hash {g.source_hash()}")
    results = []
    for nx in a.sizes:
        A, B, Cm, D = proto.plants(nx, DISTINCT)
        P = proto.pairs(A, B, Cm, D, ((0, 0),))
        t0 = time.perf_counter()
        Y = proto.samples_rk4(*P, STEPS, DT)
        info_p, _ = proto.stepinfo_batch(Y, DT)
        t_host = (time.perf_counter() - t0) / DISTINCT
        for n in a.pairs:
            reps = n // DISTINCT
            tile = lambda m: np.tile(m, (reps, 1, 1))
            w = fb.LinearWorld(proto.model(fb, tile(A), tile(B), tile(Cm), tile(D)))
            ms, info, status = timed_stepinfo(w, a.calls)
            w.close()
            same = bool(np.array_equal(info[[4, 7, 8], 0, :DISTINCT], info_p[[4, 7, 8]], equal_nan=True))
            med = float(np.median(ms))
            fma = 2.0 * (4 * STEPS + 1) * proto.group(nx) * proto.group(nx) * n      # two passes x (4 N + 1) exchanges x P FMAs on P lanes
            log(f"nx {nx:2d} P={proto.group(nx):2d} pairs {n:8d}: kernel median {med:9.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
                f"{n / (med * 1e-3):.3e} pairs/s | {fma / (med * 1e-3) / 1e12:.2f} T lane-FMA/s | status != 0: {int((status != 0).sum())} | times equal "
                f"to the prototype's: {same} | numpy host loop {t_host * 1e3:.1f} ms per system ({DISTINCT} timed) = {t_host * n:.1f} s for the batch, "
                f"{t_host * n / (med * 1e-3):.0f} x the kernel")
            results.append(dict(nx=nx, P=proto.group(nx), pairs=n, ms=[round(float(v), 4) for v in ms], pairs_per_s=n / (med * 1e-3), host_s_per_system=t_host))
    log(json.dumps({"bench_stepinfo": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
