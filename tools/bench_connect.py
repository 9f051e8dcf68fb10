#!/usr/bin/env python3
"""Closing loops on the device: kernel time of fbc::k_connect (python3 tools/bench_connect.py [--small] [--out FILE]).

1 048 576 Cessna172Xv2(NED) are trimmed and linearised on the device; the plants are built from that result device to device
(flightbatch.linear_world) in two shapes, the full 20 / 4 / 38 model and an 8 / 2 / 8 longitudinal subsystem, and each is connected with an
integrator behind three of its outputs (q, θ, EAS feed the elevator command, the integrator takes q - w): 21 / 1 / 39 and 9 / 1 / 9. The
kernel's time comes from the HIP events fb_timing_begin_per_launch puts around it on the plant's stream; the whole call (staging, the
kernel, k_lss_gather into the new handle, its allocation) is wall time. Beside them the host route the tree's examples take: model() and
model_cd() home, the block matrices in numpy, LinearWorld(...) back, on a slice of the same plants (its time is linear in N; a million full
models are 11 GB of host arrays)."""
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
from bench_lss import linearize_on_device  # noqa: E402

LON8 = ("q", "θ", "v_x", "v_z", "α_filt", "thr_p", "ele_p")
SHAPES = (("20/4/38", {}), ("8/2/8", dict(x=LON8 + ("ω_eng",), u=("throttle_cmd", "elevator_cmd"), y=LON8 + ("EAS",))))
K_Q, K_TH, K_EAS, K_XI = 0.8, 1.5, 0.01, 2.0


def wiring(plant):
    """(reads, F, G): elevator_cmd = -K_Q q - K_TH θ - K_EAS EAS + K_XI ξ, ξ' = w - q; batch-wide gains"""
    nu = plant.nu
    F = np.zeros((nu + 1, 4))
    F[plant.u_labels.index("elevator_cmd")] = (-K_Q, -K_TH, -K_EAS, K_XI)
    F[nu, 0] = -1.0
    G = np.zeros((nu + 1, 1)); G[nu, 0] = 1.0
    return ["q", "θ", "EAS", "ξ"], F, G


def kernel_ms(plant):
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(plant._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(plant._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(plant._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64)


def host_route(plant, reads, F, G):
    """the same interconnection by the route the examples take; returns (seconds home, seconds numpy, seconds back)"""
    t0 = time.perf_counter()
    A, B = plant.model()
    Cm, D = plant.model_cd()
    t1 = time.perf_counter()
    n, nx, nu, ny = plant.n, plant.nx, plant.nu, plant.ny
    As = np.zeros((n, nx + 1, nx + 1)); As[:, :nx, :nx] = A
    Bs = np.zeros((n, nx + 1, nu + 1)); Bs[:, :nx, :nu] = B; Bs[:, nx, nu] = 1.0
    Cs = np.zeros((n, ny + 1, nx + 1)); Cs[:, :ny, :nx] = Cm; Cs[:, ny, nx] = 1.0
    Ds = np.zeros((n, ny + 1, nu + 1)); Ds[:, :ny, :nu] = D
    jz = [plant.y_labels.index(r) for r in reads[:3]] + [ny]
    E = np.linalg.inv(np.eye(nu + 1) - F @ Ds[:, jz])
    M, Nw = E @ (F @ Cs[:, jz]), E @ G
    z = np.zeros
    lss = fb.LinearizedSS(xdot0=z((n, nx + 1)), x0=z((n, nx + 1)), u0=z((n, 1)), y0=z((n, ny + 1)), A=As + Bs @ M, B=Bs @ Nw, C=Cs + Ds @ M,
                          D=Ds @ Nw, x_labels=plant.x_labels + ("ξ",), u_labels=("w",), y_labels=plant.y_labels + ("ξ",))
    t2 = time.perf_counter()
    w = fb.LinearWorld(lss)
    w.sync()
    t3 = time.perf_counter()
    w.close()
    return t1 - t0, t2 - t1, t3 - t2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1/16 of the batch (a quick look)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = (1 << 20) // (16 if a.small else 1)
    nh = 65536 // (16 if a.small else 1)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_connect.py{' --small' if a.small else ''}: N = {n}, 1 warm-up + {a.calls} timed calls; source hash {g.source_hash()}")
    rng = np.random.default_rng(0)
    results = []
    for nn, host in ((n, False), (nh, True)):
        w = fb.Cessna172Xv2World(nn, kinematics="NED")
        ok = linearize_on_device(w, fb.TrimParameters(EAS=rng.uniform(35, 55, nn), h_e=rng.uniform(200, 3000, nn)).pack(nn))
        if not host:
            log(f"# trimmed {ok.mean():.4f} of the batch; the plants below are built from that result on the device")
        integ = fb.integrator_world(nn)
        for name, sel in SHAPES:
            plant = fb.linear_world(w, **sel)
            reads, F, G = wiring(plant)
            if host:
                home, npy, back = host_route(plant, reads, F, G)
                scale = n / nn
                log(f"{name:8s} + 1/s host route (N = {nn}): model home {home:.3f} s, numpy {npy:.3f} s, LinearWorld back {back:.3f} s; "
                    f"at N = {n}: {scale * (home + npy + back):.1f} s")
                results.append(dict(shape=name, route="host", n=nn, home_s=home, numpy_s=npy, back_s=back))
            else:
                wall = []
                for k in range(a.calls + 1):
                    if k == 1:
                        check(fb.lib.fb_timing_begin_per_launch(plant._h, a.calls))
                    t0 = time.perf_counter()
                    res = fb.connect(plant, integ, feedback=F, inputs=G, reads=reads, input_labels=("w",))
                    wall.append(time.perf_counter() - t0)
                    good = int(res.ok.sum())
                    res.world.close()
                ms = kernel_ms(plant)
                P = 8 if plant.nx + 1 <= 8 else 16 if plant.nx + 1 <= 16 else 32
                nx1, ny1 = plant.nx + 1, plant.ny + 1
                bytes_sys = 8 * ((plant.nx + plant.nu) * (plant.nx + plant.ny) + 4 + 2 * (nx1 + ny1) * (nx1 + 1))   # sources once, the result written and staged
                log(f"{name:8s} + 1/s k_connect<{P}>: kernel median {np.median(ms):8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) | "
                    f"{n / (np.median(ms) * 1e-3):.3e} systems/s | ~{bytes_sys * n / (np.median(ms) * 1e-3) / 1e12:.2f} TB/s of model traffic | "
                    f"whole call {np.median(wall[1:]):.3f} s | ok {good} of {n}")
                results.append(dict(shape=name, route="device", n=nn, P=P, kernel_ms=[round(float(v), 4) for v in ms], call_s=[round(v, 4) for v in wall[1:]]))
            plant.close()
        integ.close()
        w.close()
    log(json.dumps({"bench_connect": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
