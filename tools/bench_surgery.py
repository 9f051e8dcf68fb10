#!/usr/bin/env python3
"""Design-model surgery on the device: kernel time of fbm::k_transform and fbm::k_steady (python3 tools/bench_surgery.py [--n N] [--out FILE]).

N Cessna172Xv2(NED) are trimmed and linearised on the device and the 20 / 4 / 38 model is built from that result device to device
(flightbatch.linear_world). Timed, at N = 28 and at the large N:
    k_transform<32>   20 / 4 / 38 -> the longitudinal design model 9 / 2 / 16 (flightbatch.c172x_design_model(src, "lon"))
    k_transform<32>   rows = NULL: the same subsystem as a copy (flightbatch.subsystem_world)
    k_steady<16>      nx + nz = 10: the reduced longitudinal model (8 states) with z = (throttle_cmd, EAS) and a batch-wide K
The kernel's time comes from the HIP events fb_timing_begin_per_launch puts around it on the source's stream; the whole call (staging, the
kernel, k_lss_gather into the new handle and its allocation, or the results' way home) is wall time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
from bench_connect import kernel_ms  # noqa: E402
from bench_lss import linearize_on_device  # noqa: E402


def timed(world, calls, run):
    """(kernel ms of the timed calls, wall seconds of the timed calls, the last result) of 1 warm-up + `calls` calls of run()"""
    wall, res = [], None
    for k in range(calls + 1):
        if k == 1:
            check(fb.lib.fb_timing_begin_per_launch(world._h, calls))
        t0 = time.perf_counter()
        res = run(res)
        wall.append(time.perf_counter() - t0)
    return kernel_ms(world), wall[1:], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18, help="the large batch")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_surgery.py: N = 28 and {a.n}, 1 warm-up + {a.calls} timed calls; source hash {g.source_hash()}")
    rng = np.random.default_rng(0)
    results = []
    lon = ("q", "θ", "EAS", "α", "h", "α_filt", "n_eng", "thr_p", "ele_p")

    def close_then(keep):
        def run(prev):
            if prev is not None:
                (prev.world if hasattr(prev, "world") else prev).close()
            return keep()
        return run

    for n in (28, a.n):
        w = fb.Cessna172Xv2World(n, kinematics="NED")
        ok = linearize_on_device(w, fb.TrimParameters(EAS=rng.uniform(35, 55, n), h_e=rng.uniform(200, 3000, n)).pack(n))
        src = fb.linear_world(w)
        w.close()
        log(f"# N = {n}: trimmed {ok.mean():.4f} of the batch")
        ms, wall, res = timed(src, a.calls, close_then(lambda: fb.c172x_design_model(src, "lon")))
        good = int(res.ok.sum())
        # the source read once (A | B, C | D, offsets), the whole transformed model staged, the subsystem written
        bytes_sys = 8 * (2 * (24 * 58 + 82) + 11 * 25 + 22)
        log(f"N {n:8d} 20/4/38 -> lon  k_transform<32>: kernel median {np.median(ms):8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
            f"{n / (np.median(ms) * 1e-3):.3e} systems/s | ~{bytes_sys * n / (np.median(ms) * 1e-3) / 1e12:.3f} TB/s of model traffic | "
            f"whole call {np.median(wall):.4f} s | ok {good} of {n}; rpiv {np.nanmin(res.rpiv):.2e} .. {np.nanmax(res.rpiv):.2e}")
        results.append(dict(verb="transform", n=n, P=32, kernel_ms=[round(float(v), 4) for v in ms], call_s=[round(v, 4) for v in wall]))
        lon_world = res.world
        ms, wall, sub = timed(src, a.calls, close_then(lambda: fb.subsystem_world(src, x=[s for s in src.x_labels if s in ("q", "θ", "h", "α_filt", "thr_p", "ele_p")],
                                                                                   u=lon_world.u_labels, y=lon_world.y_labels)))
        sub.close()
        log(f"N {n:8d} 20/4/38 copy    k_transform<32>, rows = NULL: kernel median {np.median(ms):8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
            f"whole call {np.median(wall):.4f} s")
        results.append(dict(verb="transform, rows = NULL", n=n, P=32, kernel_ms=[round(float(v), 4) for v in ms], call_s=[round(v, 4) for v in wall]))
        red = fb.delete_vars_world(lon_world, "h")
        K = 0.1 * np.random.default_rng(1).standard_normal((2, 8))
        ms, wall, st = timed(red, a.calls, lambda prev: fb.steady_state(red, ("throttle_cmd", "EAS"), K))
        log(f"N {n:8d} nx + nz = 10    k_steady<16>:    kernel median {np.median(ms):8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
            f"{n / (np.median(ms) * 1e-3):.3e} systems/s | whole call {np.median(wall):.4f} s | ok {int(st.ok.sum())} of {n}")
        results.append(dict(verb="steady", n=n, P=16, kernel_ms=[round(float(v), 4) for v in ms], call_s=[round(v, 4) for v in wall]))
        assert tuple(lon_world.x_labels) == lon
        for x in (red, lon_world, src):
            x.close()
    log(json.dumps({"bench_surgery": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
