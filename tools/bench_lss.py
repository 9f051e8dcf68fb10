#!/usr/bin/env python3
"""Model(lss) on the device: launch times of k_lss_rk4 (python3 tools/bench_lss.py [--small] [--out FILE]).

1 048 576 Cessna172Sv0(NED) are trimmed and linearised on the device; the linear models are built from that result device to device
(flightbatch.linear_world) in two shapes: the full 16 / 4 / 33 model and the longitudinal subsystem 4 / 1 / 2 (x = q θ v_x v_z, u = elevator,
y = q θ). Each is stepped 50 RK4 steps per launch with the elevator off its trim value; per-launch HIP events come from
fb_timing_begin_per_launch, after warm-up launches as bench.py runs them. Both exchanges of the stepper are timed (FLIGHTBATCH_LSS_EXCHANGE:
the LDS panel, the default, and cross-lane reads). Beside them: the numpy RK4 of examples/elevator_step.py (linear_response's loop), the way
the same job is done without these kernels, on a slice of the same models."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402
from flightbatch import linearization as L  # noqa: E402
from flightbatch._lib import check  # noqa: E402

INNER, DT = 50, 0.02
LON = dict(x=("q", "θ", "v_x", "v_z"), u=("elevator",), y=("q", "θ"))
FP64_VALU_PEAK_TFLOPS = 78.6   # MI355X vector fp64 (bench.py's figure)


def linearize_on_device(w, tp):
    """fb_linearize with every block written on the device and only x0, u0, B, D copied back (A | B and C | D are written together)"""
    d, b, ptrs = L._buffers(w)
    n = w.n
    ts = fb.TrimState(n)
    ok = np.zeros(n, dtype=np.int32)
    cost = np.zeros(n)
    keep = [None, ptrs[1], ptrs[2], None, None, ptrs[5], None, ptrs[7], ptrs[8]]
    _pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    check(fb.lib.fb_linearize(w._h, _pd(tp), _pd(ts), ok.ctypes.data_as(C.POINTER(C.c_int32)), _pd(cost), fb.K["FB_LIN_FORWARD"], *keep))
    return ok


def time_launches(lw, warmup, launches):
    check(fb.lib.fb_set_steps_per_launch(lw._h, INNER))
    lw.set_params(dt=DT)
    for _ in range(warmup):
        lw.step(INNER)
    lw.sync()
    check(fb.lib.fb_timing_begin_per_launch(lw._h, launches))
    for _ in range(launches):
        lw.step(INNER)
    lw.sync()
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(lw._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(lw._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(lw._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64)


def host_rk4_rate(lss, steps):
    """system-steps per second of linear_response's loop (examples/elevator_step.py): einsum A x + B a, classical RK4"""
    n = lss.A.shape[0]
    A, B = lss.A, lss.B[:, :, 0]
    a = np.full(n, 0.05)
    f = lambda x: np.einsum("nij,nj->ni", A, x) + B * a[:, None]
    x = np.zeros((n, A.shape[1]))
    t0 = time.perf_counter()
    for _ in range(steps):
        k1 = f(x); k2 = f(x + DT / 2 * k1); k3 = f(x + DT / 2 * k2); k4 = f(x + DT * k3)
        x = x + DT / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return n * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1/16 of the batch (a quick look)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = (1 << 20) // (16 if a.small else 1)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_lss.py{' --small' if a.small else ''}: N = {n}, {INNER} steps per launch, {a.warmup} warm-up + {a.launches} timed launches; source hash {g.source_hash()}")
    rng = np.random.default_rng(0)
    w = fb.BatchedWorld(n, kinematics="NED")
    tp = fb.TrimParameters(EAS=rng.uniform(35, 55, n), h_e=rng.uniform(200, 3000, n)).pack(n)
    ok = linearize_on_device(w, tp)
    log(f"# trimmed {ok.mean():.4f} of the batch; the linear models below are built from that result on the device")
    results = []
    for name, sel in (("16/4/33", {}), ("4/1/2", LON)):
        for xch in ("panel", "shfl"):
            os.environ["FLIGHTBATCH_LSS_EXCHANGE"] = xch      # (read when the handle is created)
            t0 = time.perf_counter()
            lw = fb.linear_world(w, **sel)
            t_build = time.perf_counter() - t0
            u = lw.u
            u[lw.u_labels.index("elevator")] += 0.05
            lw.u = u
            ms = time_launches(lw, a.warmup, a.launches)
            G = 4 if lw.nx <= 4 else 8 if lw.nx <= 8 else 16 if lw.nx <= 16 else 32
            rate = n * INNER / (np.median(ms) * 1e-3)
            tflops = 2 * 4 * G * (G + 1) * rate / 1e12      # 4 G (G + 1) FMAs per system-step, padding included
            finite = bool(np.isfinite(lw.x).all())
            log(f"{name:8s} G={G:2d} {xch:5s}: launch median {np.median(ms):8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
                f"{rate:.3e} system-steps/s | {tflops:6.2f} TFLOP/s fp64 = {100 * tflops / FP64_VALU_PEAK_TFLOPS:5.1f} % of the vector peak | "
                f"device-to-device build {t_build * 1e3:.0f} ms | state finite: {finite}")
            results.append(dict(shape=name, G=G, exchange=xch, ms=[round(float(v), 4) for v in ms], system_steps_per_s=rate, tflops=tflops))
            lw.close()
    os.environ.pop("FLIGHTBATCH_LSS_EXCHANGE", None)
    w.close()
    # the host loop, on 65 536 of the same kind of models (its time is linear in N; 1 048 576 full models are 8.8 GB of host arrays)
    nh = 65536 // (16 if a.small else 1)
    wh = fb.BatchedWorld(nh, kinematics="NED")
    lss = fb.linearize(wh, fb.TrimParameters(EAS=rng.uniform(35, 55, nh), h_e=rng.uniform(200, 3000, nh)))
    wh.close()
    for name, m in (("16/4/33", lss), ("4/1/2", fb.subsystem(lss, **LON))):
        rate = host_rk4_rate(m, 5)
        log(f"{name:8s} numpy RK4 on the host (N = {nh}, 5 steps): {rate:.3e} system-steps/s; a launch's work (1 048 576 x {INNER}) would take {(1 << 20) * INNER / rate:.1f} s")
        results.append(dict(shape=name, exchange="host numpy", system_steps_per_s=rate))
    log(json.dumps({"bench_lss": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
