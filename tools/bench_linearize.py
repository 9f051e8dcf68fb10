#!/usr/bin/env python3
"""fb_linearize / fb_linearize_state timing (python3 tools/bench_linearize.py [--small] [--out FILE]): for 1 048 576 Cessna172Sv0(NED) with
both schemes and 524 288 Cessna172Xv2(NED) with the forward scheme, the stream time of

  trim      the still-air trim alone (f_init: k_trim, k_kin_convert, [k_x2_init])
  lin       fb_linearize_state with only B and lin_status copied back: every linearisation kernel runs, the copy is B's bytes alone
  full      fb_linearize_state with every block copied back to pageable numpy memory
  call      fb_linearize (trim + linearisation + every copy), wall clock

Per-kernel times come from running this tool under `rocprofv3 --kernel-trace --stats -- python3 tools/bench_linearize.py`. Writes the table
to profiles/r07_linearize.txt (or --out)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402
from flightbatch import linearization as L  # noqa: E402
from flightbatch._lib import check  # noqa: E402


def _timed(w, fn):
    fb.lib.fb_timing_begin(w._h)
    fn()
    ms = C.c_float()
    check(fb.lib.fb_timing_end(w._h, C.byref(ms), None))
    return ms.value


def run(model, n, scheme, log):
    W = fb.Cessna172Xv2World if model == "Xv2" else fb.BatchedWorld
    w = W(n, kinematics="NED")
    rng = np.random.default_rng(0)
    tp = fb.TrimParameters(EAS=rng.uniform(30, 55, n), h_e=rng.uniform(200, 3000, n), flaps=rng.uniform(0, 0.5, n))
    lss = L.linearize(w, tp, scheme=scheme)            # (first call: device buffers allocated)
    t0 = time.perf_counter()
    lss = L.linearize(w, tp, scheme=scheme)
    t_call = time.perf_counter() - t0
    ms_trim = _timed(w, lambda: fb.f_init(w, tp))
    d, b, ptrs = L._buffers(w)
    nx, nu, ny = d
    s = fb.K["FB_LIN_" + ("FORWARD" if scheme == "forward" else "ONESIDED2")]
    only_b = [None] * 5 + [ptrs[5]] + [None] * 2 + [ptrs[8]]
    ms_lin_b = _timed(w, lambda: check(fb.lib.fb_linearize_state(w._h, s, *only_b)))
    ms_full = _timed(w, lambda: check(fb.lib.fb_linearize_state(w._h, s, *ptrs)))
    per = 8 * (2 * nx + nu + ny + (nx + ny) * (nx + nu))
    ok = lss.success.mean()
    line = (f"{model:4s} N={n:8d} {scheme:9s}: trim {ms_trim:8.2f} ms | linearisation kernels + copy of B ({8 * nx * nu * n / 1e9:.2f} GB) "
            f"{ms_lin_b:8.2f} ms | fb_linearize_state, every block copied ({per * n / 1e9:.2f} GB) {ms_full:8.2f} ms | "
            f"fb_linearize wall {t_call * 1e3:8.1f} ms | trimmed {ok:.4f}")
    log(line)
    w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="1/16 of the sizes (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_linearize.txt"))
    a = ap.parse_args()
    k = 16 if a.small else 1
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log(f"# tools/bench_linearize.py{' --small' if a.small else ''} — source hash of the build: see __graft_entry__.source_hash()")
    import __graft_entry__ as g  # noqa: E402
    log(f"# source hash {g.source_hash()}")
    run("Sv0", (1 << 20) // k, "forward", log)
    run("Sv0", (1 << 20) // k, "onesided2", log)
    run("Xv2", (1 << 19) // k, "forward", log)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
