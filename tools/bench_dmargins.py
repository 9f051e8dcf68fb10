#!/usr/bin/env python3
"""Sampled loops on the device: kernel times of fb_lss_dmargins beside fb_lss_margins (python3 tools/bench_dmargins.py [--out FILE]).

Two sides in one run: the continuous plants of tools/bench_margins.py (K / (s + 1)³ with K = 2, 4, 7 among nx = 4, 9, 20 states behind a
random orthogonal change of state, 64 distinct ones tiled over 4096 and 1 048 576 systems) on pidopt.default_grid(), and their
zero-order hold at Ts = 0.02 (fb_lss_c2d) on default_dgrid(Ts), 321 frequencies each. A call of either verb is its grid response
(k_lss_freqresp / k_lss_dfreqresp, the sum over the slices) and then its margins kernel (k_lss_margins / k_lss_dmargins), each launch
between its own pair of HIP events (fb_timing_begin_per_launch). After one warm-up of each side the calls alternate, continuous then
sampled; the medians and their ratios are printed. From the operation counts alone the ratios should be near 1: the same FMAs per
elimination, one division and one square root per halving where the continuous kernel has a square root. Nothing gates on these numbers."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
import margins_prototype as proto  # noqa: E402

NX_ALL, SYSTEMS, DISTINCT, CALLS, TS = (4, 9, 20), (4096, 1 << 20), 64, 3, 0.02


def stamps(w, calls):
    """the per-launch times of the window on w as [calls, 2] in ms: the grid response (the sum over its slices), the margins kernel"""
    ms, nl = C.c_float(), C.c_int64()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
    check(fb.lib.fb_timing_launches(w._h, None, 0, C.byref(nl)))
    buf = (C.c_float * nl.value)()
    check(fb.lib.fb_timing_launches(w._h, buf, nl.value, C.byref(nl)))
    ms = np.array(buf[:nl.value], dtype=np.float64).reshape(calls, -1)
    return np.stack([ms[:, :-1].sum(axis=1), ms[:, -1]], axis=1), ms.shape[1] - 1


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
    wc, wd = fb.pidopt.default_grid(), fb.default_dgrid(TS)
    log(f"# tools/bench_dmargins.py: K / (s + 1)^3 among nx states, {DISTINCT} distinct systems tiled; continuous on {wc.size} frequencies, "
        f"their zero-order hold at Ts = {TS:g} on {wd.size}; 1 warm-up + {a.calls} timed calls of each verb, alternating; source hash {g.source_hash()}")
    results = []
    for nx in NX_ALL:
        rng = np.random.default_rng(nx)
        systems = [proto.embed(proto.cube(proto.K_CLOSED[k % 3]), nx, rng) for k in range(DISTINCT)]
        M = proto.lss_arrays(systems, nu=1, ny=1, iu=0, iy=0)
        for n in a.systems:
            reps = n // DISTINCT
            tile = lambda m: np.tile(m, (reps,) + (1,) * (m.ndim - 1))
            cont = fb.LinearWorld(fb.LinearizedSS(**{k: tile(v) for k, v in M.items()}, x_labels=tuple(f"x{k}" for k in range(nx)),
                                                  u_labels=("u",), y_labels=("y",)))
            held = fb.c2d(cont, TS)
            assert (held.status == 0).all()
            rc, rd = fb.margins(cont, w=wc), fb.dmargins(held.world, w=wd)
            for w in (cont, held.world):
                check(fb.lib.fb_timing_begin_per_launch(w._h, 64 * a.calls))
            for _ in range(a.calls):
                fb.margins(cont, w=wc)
                fb.dmargins(held.world, w=wd)
            (mc, sc), (md, sd) = stamps(cont, a.calls), stamps(held.world, a.calls)
            cont.close(); held.world.close()
            med = lambda v: float(np.median(v))
            c1, c2, d1, d2 = med(mc[:, 0]), med(mc[:, 1]), med(md[:, 0]), med(md[:, 1])
            log(f"nx = {nx:2d}, N = {n:7d}: k_lss_freqresp ({sc}) {c1:9.3f} ms, k_lss_dfreqresp ({sd}) {d1:9.3f} ms, ratio {d1 / c1:.3f} | "
                f"k_lss_margins {c2:9.3f} ms, k_lss_dmargins {d2:9.3f} ms, ratio {d2 / c2:.3f} | crossings per system {float((rc.npc + rc.ngc).mean()):.2f} "
                f"and {float((rd.npc + rd.ngc).mean()):.2f}, status != 0: {int((rc.status != 0).sum())} and {int((rd.status != 0).sum())}")
            results.append(dict(nx=nx, n=n, slices=[sc, sd], freqresp_ms=[round(float(v), 4) for v in mc[:, 0]], dfreqresp_ms=[round(float(v), 4) for v in md[:, 0]],
                                margins_ms=[round(float(v), 4) for v in mc[:, 1]], dmargins_ms=[round(float(v), 4) for v in md[:, 1]]))
    log(json.dumps({"bench_dmargins": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
