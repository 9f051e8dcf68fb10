#!/usr/bin/env python3
"""The five LQR tables of the reference's autopilot (design_lon, design_lat: lib/FlightApps/design/c172/c172x_design.jl:134-700) for
Cessna172Xv2(NED) at its 28 design nodes, from trim to K_fbk, K_fwd and K_int with no model coming home.

    trim + linearize at every (EAS, h) node                  fb.linearize(world, TrimParameters(...))      on the device
    Model(lss)                                               fb.linear_world(world)                        device to device
    get_design_model!(ac, trim; model = :lon / :lat)         fb.c172x_design_model(src, "lon" / "lat")     on the device   (:23-82)
    delete_vars(lss_lon, :h), delete_vars(lss_lat, :ψ)       fb.delete_vars_world(...)                     device to device (:144, :559)
    A_aug, B_aug; K = lqr(P_aug, Q, R)                       fb.lqr_tracker -> integral_augmentation, lqr  on the device   (:354-369)
    M = inv([A B; C D]); K_fwd = M22 + K_fbk M12             fb.lqr_tracker -> steady_state                on the device   (:184-188)

Only the gains cross the bus (K_fbk goes back up for K_fwd). The tables are compared with the ones the product ships
(flight.jl_amd/data/c172x_ctl/*.h5). `python examples/tracker_schedule.py [device]`"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains  # noqa: E402
from lqr_schedule import flaps_schedule  # noqa: E402

# name: (model, deleted state, z, Q diagonal on the states, Q diagonal on the integrators, R diagonal, K_fwd rule)
DESIGNS = {
    "te2te": ("lon", "h", ("throttle_cmd", "elevator_cmd"), dict(q=1, θ=20, EAS=0.02), None, (100, 5), "inverse"),                 # :173-188
    "tv2te": ("lon", "h", ("throttle_cmd", "EAS"), dict(q=20, EAS=0.3), (0.1, 0.01), (1, 0.1), "inverse"),                         # :362-382
    "vh2te": ("lon", None, ("EAS", "h"), dict(q=20, θ=100, EAS=0.06, h=0.04), (0.005, 0.001), (0.1, 0.05), "inverse"),             # :469-488
    "ar2ar": ("lat", "ψ", ("aileron_cmd", "rudder_cmd"), dict(r=0.1, φ=0.1), None, (0.1, 0.01), "identity"),                       # :584-594
    "phibeta2ar": ("lat", "ψ", ("φ", "β"), dict(r=0.1, φ=2, β=5), None, (0.1, 0.03), "inverse"),                                        # :646-675
}


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    stored = {name: ctl_gains.load_lqr(os.path.join(ctl_gains.DATA_DIR, name + ".h5")) for name in DESIGNS}
    (e0, e1), (h0, h1) = stored["te2te"]["bounds"].T
    nE, nH = stored["te2te"]["K_fbk"].shape[-2:]
    E, H = np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij")
    EAS, h = E.ravel(order="F"), H.ravel(order="F")
    n = EAS.size

    w = fb.Cessna172Xv2World(n, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps_schedule(EAS)), scheme="onesided2")
    src = fb.linear_world(w)
    w.close()

    t0 = time.perf_counter()
    models = {m: fb.c172x_design_model(src, m) for m in ("lon", "lat")}
    worlds = {}
    print(f"{n} nodes: trimmed {int(lss.success.sum())}; design models ok {int(models['lon'].ok.sum())}, rpiv of T {models['lon'].rpiv.min():.2e} .. "
          f"{models['lon'].rpiv.max():.2e}")
    for name, (model, drop, z, qx, qi, r, fwd) in DESIGNS.items():
        if (model, drop) not in worlds:
            worlds[model, drop] = models[model].world if drop is None else fb.delete_vars_world(models[model].world, drop)
        P = worlds[model, drop]
        q = [float(qx.get(s, 0.0)) for s in P.x_labels]
        K_fbk, K_fwd, K_int, status = fb.lqr_tracker(P, z, q, np.array(r, dtype=np.float64), qi, forward=fwd, device=device)
        st = stored[name]
        dev = []
        for got, key in ((K_fbk, "K_fbk"), (K_fwd, "K_fwd"), (K_int, "K_int")):
            want = np.moveaxis(st[key].reshape(st[key].shape[:2] + (-1,), order="F"), -1, 0)
            scale = np.abs(want).max() or 1.0
            dev.append(np.abs(got - want).max() / scale)
        print(f"{name:10s} states {P.nx}{'' if qi is None else ' + ' + str(len(qi)) + ' integrators'}: designed {int((status == 0).sum())} of {n}; "
              f"vs the shipped table K_fbk {dev[0]:.1e}  K_fwd {dev[1]:.1e}  K_int {dev[2]:.1e}")
    print(f"design models to the last table: {time.perf_counter() - t0:.2f} s")
    for x in set(worlds.values()) | {models["lon"].world, models["lat"].world, src}:
        x.close()


if __name__ == "__main__":
    main()
