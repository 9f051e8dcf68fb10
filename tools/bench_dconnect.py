#!/usr/bin/env python3
"""Closing sampled loops on the device: kernel time of fbv::k_dconnect beside fbc::k_connect (python3 tools/bench_dconnect.py [--out FILE]).

The two shapes of tools/bench_connect.py, at N = 4096 and N = 1 048 576: Cessna172Xv2(NED) trimmed and linearised on the device, the full
20 / 4 / 38 model and the 8 / 2 / 8 longitudinal subsystem, each with an integrator behind q, θ and EAS (bench_connect.wiring). Every plant
is built twice from the same linearisation (flightbatch.linear_world): one stays continuous and goes through fb_lss_connect, the other is
marked sampled (fb_lss_set_sampled: the same four matrices, read as Phi and Gamma) and goes through fb_lss_dconnect with nd = 0 and with
nd = nu_p (the first nu_p reads taken one sample late). What is timed is arithmetic on the same numbers, not a discretisation. The three
run in one process, alternating, after one warm-up round; the figure is the median of the timed rounds' kernel times, from the HIP events
fb_timing_begin_per_launch puts around each kernel on its plant's stream. With nd = 0 the four matrices must come out bit for bit as
fb_lss_connect's: checked here on a slice of the batch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flightbatch as fb  # noqa: E402
from flightbatch._lib import check  # noqa: E402
from bench_connect import SHAPES, kernel_ms, wiring  # noqa: E402
from bench_lss import linearize_on_device  # noqa: E402

TS = 0.02
group = lambda rows: 8 if rows <= 8 else 16 if rows <= 16 else 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 1 << 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    import __graft_entry__ as g
    log(f"# tools/bench_dconnect.py: 1 warm-up + {a.rounds} timed rounds, alternating connect | dconnect nd = 0 | dconnect nd = nu_p; kernel ms, "
        f"median (min, max); source hash {g.source_hash()}")
    rng = np.random.default_rng(0)
    results = []
    for n in a.sizes:
        w = fb.Cessna172Xv2World(n, kinematics="NED")
        ok = linearize_on_device(w, fb.TrimParameters(EAS=rng.uniform(35, 55, n), h_e=rng.uniform(200, 3000, n)).pack(n))
        log(f"# N = {n}: trimmed {ok.mean():.4f} of the batch")
        integ, dinteg = fb.integrator_world(n), fb.integrator_world(n)
        check(fb.lib.fb_lss_set_sampled(dinteg._h, TS))
        for name, sel in SHAPES:
            plant, dplant = fb.linear_world(w, **sel), fb.linear_world(w, **sel)
            check(fb.lib.fb_lss_set_sampled(dplant._h, TS))
            reads, F, G = wiring(plant)
            nd = plant.nu
            late = reads[:nd]
            dreads = [r + "[k-1]" for r in late] + reads[nd:]
            same = None
            for k in range(a.rounds + 1):
                if k == 1:
                    check(fb.lib.fb_timing_begin_per_launch(plant._h, a.rounds))
                    check(fb.lib.fb_timing_begin_per_launch(dplant._h, 2 * a.rounds))
                rc = fb.connect(plant, integ, feedback=F, inputs=G, reads=reads, input_labels=("w",))
                r0 = fb.dconnect(dplant, dinteg, feedback=F, inputs=G, reads=reads, input_labels=("w",))
                r1 = fb.dconnect(dplant, dinteg, feedback=F, inputs=G, delays=late, reads=dreads, input_labels=("w",))
                good = (int(rc.ok.sum()), int(r0.ok.sum()), int(r1.ok.sum()))
                if k == 0 and n <= 4096:      # (the whole models come home: on the small batch only)
                    same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(rc.world.model() + rc.world.model_cd(), r0.world.model() + r0.world.model_cd()))
                for r in (rc, r0, r1):
                    r.world.close()
            mc, md = kernel_ms(plant), kernel_ms(dplant)
            m0, m1 = md[0::2], md[1::2]
            nx1 = plant.nx + 1
            fmt = lambda m: f"{np.median(m):8.3f} ({m.min():.3f}, {m.max():.3f})"
            log(f"N {n:8d} {name:8s} + 1/s | k_connect<{group(nx1)}> {fmt(mc)} | k_dconnect<{group(nx1)}> nd = 0 {fmt(m0)}, ratio {np.median(m0) / np.median(mc):.3f} | "
                f"k_dconnect<{group(nx1 + nd)}> nd = {nd} (nx' = {nx1 + nd}) {fmt(m1)}, ratio {np.median(m1) / np.median(mc):.3f} | ok {good} of {n}"
                + ("" if same is None else f" | nd = 0 bits equal connect's: {same}"))
            results.append(dict(n=n, shape=name, nd=nd, connect_ms=[round(float(v), 4) for v in mc], dconnect_nd0_ms=[round(float(v), 4) for v in m0],
                                dconnect_nd_ms=[round(float(v), 4) for v in m1], bits_equal=same))
            plant.close(); dplant.close()
        integ.close(); dinteg.close()
        w.close()
    log(json.dumps({"bench_dconnect": results}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
