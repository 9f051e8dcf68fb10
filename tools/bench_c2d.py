#!/usr/bin/env python3
"""Sampled models on the device: kernel times of k_lss_c2d and of k_timeresp_map beside k_timeresp
(python3 tools/bench_c2d.py [--systems N ...] [--sizes NX ...] [--out FILE]).

For nx = 4, 9, 20 at 4096 and 1 048 576 systems (the random stable plants of tests/timeresp_prototype.py, 64 distinct ones tiled over the
batch): fb_lss_c2d at Ts = 1e-3 (s = 0) and at Ts = 0.25 (s = 2 .. 3), and fb_lss_stepinfo (info only, no sample buffer, one channel, 5000
steps per pass: the configuration of tools/bench_stepinfo.py) on the continuous world (k_timeresp, RK4: 4 N + 1 exchanges per pass) and on
the sampled one (k_timeresp_map: N + 1). HIP events around the kernels from fb_timing_begin_per_launch, the median of 3 calls after one
warm-up. Nothing is asserted; the figures go to profiles/c2d_bench.txt and docs/design/linearize.md."""
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
import timeresp_prototype as proto  # noqa: E402

SIZES = [4, 9, 20]
SYSTEMS = [4096, 1 << 20]
STEPS, DT = 5000, 1e-3
C2D_TS = [1e-3, 0.25]
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


def timed_c2d(w, Ts, calls):
    squarings = []

    def run():
        res = fb.c2d(w, Ts)
        squarings.append(int(res.squarings.max()))
        assert res.ok.all()
        res.world.close()
    return stamps(w, calls, run), squarings[-1]


def timed_stepinfo(w, calls):
    n = w.n
    ch = np.zeros(1, dtype=np.int32)
    info, status = np.empty((9, 1, n)), np.empty((1, n), dtype=np.int32)
    run = lambda: check(fb.lib.fb_lss_stepinfo(w._h, _pi(ch), _pi(ch), 1, STEPS * DT, DT, None, None, None, 1, None, _pd(info), _pi(status)))
    return stamps(w, calls, run), info.copy(), status.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--systems", type=int, nargs="+", default=SYSTEMS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_c2d.py: 1 warm-up + {a.calls} timed calls, medians; stepinfo: {STEPS} steps per pass, two passes, info only, one channel; "
        f"source hash {g.source_hash()}")
    results = []
    for nx in a.sizes:
        A, B, Cm, D = proto.plants(nx, DISTINCT)
        for n in a.systems:
            reps = n // DISTINCT
            tile = lambda m: np.tile(m, (reps, 1, 1))
            w = fb.LinearWorld(proto.model(fb, tile(A), tile(B), tile(Cm), tile(D)))
            rec = dict(nx=nx, systems=n)
            for Ts in C2D_TS:
                ms, s = timed_c2d(w, Ts, a.calls)
                med = float(np.median(ms))
                P = 8 if nx <= 8 else 16 if nx <= 16 else 32
                log(f"k_lss_c2d      nx {nx:2d} P={P:2d} systems {n:8d} Ts {Ts:g} (s <= {s}): kernel median {med:9.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
                    f"{n / (med * 1e-3):.3e} systems/s")
                rec[f"c2d_ms_Ts{Ts:g}"] = [round(float(v), 4) for v in ms]
            ms_rk4, info_rk4, st_rk4 = timed_stepinfo(w, a.calls)
            sw = fb.c2d(w, DT).world
            ms_map, info_map, st_map = timed_stepinfo(sw, a.calls)
            sw.close()
            w.close()
            m_rk4, m_map = float(np.median(ms_rk4)), float(np.median(ms_map))
            same = bool(np.array_equal(info_rk4[[4, 7, 8]], info_map[[4, 7, 8]], equal_nan=True))
            P = proto.group(nx)
            log(f"k_timeresp     nx {nx:2d} P={P:2d} pairs   {n:8d}: kernel median {m_rk4:9.3f} ms (min {ms_rk4.min():.3f}, max {ms_rk4.max():.3f})")
            log(f"k_timeresp_map nx {nx:2d} P={P:2d} pairs   {n:8d}: kernel median {m_map:9.3f} ms (min {ms_map.min():.3f}, max {ms_map.max():.3f}) | "
                f"{m_map / m_rk4:.3f} of k_timeresp (exchanges: {(STEPS + 1) / (4 * STEPS + 1):.3f}) | status != 0: {int((st_map != 0).sum())} | "
                f"times equal to RK4's: {same}")
            rec.update(timeresp_ms=[round(float(v), 4) for v in ms_rk4], timeresp_map_ms=[round(float(v), 4) for v in ms_map], ratio=m_map / m_rk4)
            results.append(rec)
    log(json.dumps({"bench_c2d": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
