#!/usr/bin/env python3
"""Discrete LQR trackers on the device: k_dtracker against timeresp.step on the dtracker_world loop (python3 tools/bench_dtracker.py
[--systems N ...] [--out FILE]).

k_dtracker steps one candidate per system under the flown law, clamp and halt logic included, and delivers every command variable, every
input, their metrics and counts. The second side is what the verbs before it could do, for the unbounded law only: the loop closed by
dconnect (dtracker_world, states [x; ι]) and stepped by fb_lss_stepinfo, one launch for the nz channels zref_c -> z_c. Plants: a lag chain
with nx = 4 and nx = 12 states, two inputs, two command variables and C = I on the states (the loop world reads x from the outputs), 256
distinct ones tiled over batches of 4096 and 2^20 systems; 4096 ticks at Ts = 0.02, only the first and the last sample come home. Both sides
run in one process, alternating after a warm-up call each; every launch sits between its own pair of HIP events
(fb_timing_begin_per_launch), and the time quoted is the kernel's alone. Nothing gates on these numbers."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, ROOT)
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402

N_TICKS, TS, DISTINCT = 4096, 0.02, 256


def stamps(w):
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    return np.array(buf[:nl.value], dtype=np.float64)


def plants(nx, n):
    """Phi, Gamma, C, D of a chain of lags with two inputs; the outputs are the states, z = (x_0, x_nx-1)"""
    rng = np.random.default_rng(nx)
    pole = 0.80 + 0.15 * rng.random((n, nx))
    Phi = np.zeros((n, nx, nx))
    k = np.arange(nx)
    Phi[:, k, k] = pole
    Phi[:, k[1:], k[:-1]] = 0.05
    Gam = np.zeros((n, nx, 2))
    Gam[:, 0, 0] = 0.1
    Gam[:, nx - 1, 1] = 0.1
    return Phi, Gam, np.broadcast_to(np.eye(nx), (n, nx, nx)).copy(), np.zeros((n, nx, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--systems", type=int, nargs="*", default=[4096, 1 << 20])
    ap.add_argument("--nx", type=int, nargs="*", default=[4, 12])
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
    log(f"# tools/bench_dtracker.py: one candidate per system, nu = nz = 2, {N_TICKS} ticks at Ts = {TS}; 1 warm-up + {a.calls} timed calls a side, "
        f"alternating; source hash {g.source_hash()}")
    results = []
    z = np.zeros
    for n, nx in ((n, nx) for n in a.systems for nx in a.nx):
        Phi, Gam, Cm, D = plants(nx, DISTINCT)
        idx = np.arange(n) % DISTINCT
        xl = tuple(f"x{k}" for k in range(nx))
        lss = fb.LinearizedSS(xdot0=z((n, nx)), x0=z((n, nx)), u0=z((n, 2)), y0=z((n, nx)), A=Phi[idx], B=Gam[idx], C=Cm[idx], D=D[idx],
                              x_labels=xl, u_labels=("u0", "u1"), y_labels=xl)
        w = fb.LinearWorld(lss, Ts=TS)
        zl = [xl[0], xl[-1]]
        K_fbk = np.zeros((2, nx)); K_fbk[0, 0] = K_fbk[1, nx - 1] = 0.5
        K_fwd, K_int = 0.5 * np.eye(2), 2.0 * np.eye(2)
        zref = np.array([1.0, -0.5])
        loop = fb.dtracker_world(w, zl, K_fbk, K_fwd, K_int)
        law = lambda: fb.dtracker_metrics(w, zl, K_fbk, K_fwd, K_int, zref, N_TICKS * TS)
        old = lambda: fb.timeresp.step(loop, [(f"{zl[0]}_ref", zl[0]), (f"{zl[1]}_ref", zl[1])], N_TICKS * TS, stride=N_TICKS)
        rl, ro = law(), old()
        check(fb.lib.fb_timing_begin_per_launch(w._h, a.calls))
        check(fb.lib.fb_timing_begin_per_launch(loop._h, a.calls))
        for _ in range(a.calls):
            law()
            old()
        tl, to = stamps(w), stamps(loop)
        w.close()
        loop.close()
        ml, mo = float(np.median(tl)), float(np.median(to))
        log(f"N = {n:7d}, nx = {nx:2d}: k_dtracker median {ml:9.3f} ms (min {tl.min():.3f}, max {tl.max():.3f}) | fb_lss_stepinfo on the loop world "
            f"(nx + nu = {nx + 2} states, 2 channels) median {mo:9.3f} ms (min {to.min():.3f}, max {to.max():.3f}) | ratio {mo / ml:.2f} | "
            f"{n * N_TICKS / (ml * 1e-3):.3e} pair-ticks/s | status != 0: {int((rl.status != 0).sum())}, {int((ro.status != 0).sum())}")
        results.append(dict(nx=nx, systems=n, ticks=N_TICKS, dtracker_ms=[round(float(v), 4) for v in tl], stepinfo_ms=[round(float(v), 4) for v in to]))
    log(json.dumps({"bench_dtracker": results}))


if __name__ == "__main__":
    main()
