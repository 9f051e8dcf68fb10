#!/usr/bin/env python3
"""The LQR trackers under the law as it flies: the reference's stored tv2te, vh2te and φβ2ar gains were designed in continuous time
(examples/tracker_schedule.py; design_lon, design_lat: lib/FlightApps/design/c172/c172x_design.jl:328-700), but Cessna172Xv2 runs the
sampled tracker (f_periodic! of LQR, FP/control.jl:708-743) every Δt = 0.02, with its outputs clamped to the actuator range and an
integrator that halts while clamped. At the 28 design nodes:

    the design models, as examples/tracker_schedule.py builds them     fb.linearize, fb.c172x_design_model, fb.delete_vars_world   on the device
    their zero-order hold at Ts = 0.02                                  fb.c2d(world, 0.02)                                         on the device
    the stored gains, continuous loop                                   fb.connect, fb.timeresp.step (the laws with D_z = 0)           on the device
    the stored gains under the flown law, unbounded and bounded         fb.dtracker_metrics(world, z, K_fbk, K_fwd, K_int, zref, t_sim, bounds=...)
    the gains designed for 50 Hz (the laws with D_z = 0)                fb.dlqr_tracker(world, z, Q, R, Q_int)

The bounds are the flown blocks': throttle_cmd in [0, 1], elevator_cmd, aileron_cmd and rudder_cmd in [-1, 1], here as bounds on the
deviation from the stored u_trim. tv2te commands throttle_cmd itself (D_z != 0): the flown law reads last tick's, dtracker_metrics serves
it, and dlqr_tracker flags it DIRECT instead of designing it. `python examples/dtracker_schedule.py [device]`"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import flightbatch as fb  # noqa: E402
from flightbatch import ctl_gains  # noqa: E402
from lqr_schedule import flaps_schedule  # noqa: E402
from tracker_schedule import DESIGNS  # noqa: E402

TS = 0.02
# name: (the step of the reference in z's units, t_sim, the flown block's output range)
STEPS = {"tv2te": ((0.1, 2.0), 10.0, ((0.0, -1.0), (1.0, 1.0))), "vh2te": ((2.0, 10.0), 20.0, ((0.0, -1.0), (1.0, 1.0))),
         "phibeta2ar": ((0.3, 0.05), 8.0, ((-1.0, -1.0), (1.0, 1.0)))}


def continuous_response(cont, z, K_fbk, K_fwd, K_int, zref, t_sim, device):
    """z(t) [N, nz, ns] of the continuous loop u = ι + K_fwd zref - K_fbk x, ι' = K_int (zref - z), by connect and timeresp.step (RK4 at Ts / 4)"""
    n, nx, nu, nz = cont.n, cont.nx, cont.nu, len(z)
    ix = [cont.y_labels.index(s) for s in cont.x_labels]
    iz = [cont.y_labels.index(s) for s in z]
    F = np.zeros((n, 2 * nu, nx + nz + nu)); G = np.zeros((n, 2 * nu, nz))
    F[:, :nu, :nx] = -K_fbk; F[:, :nu, nx + nz:] = np.eye(nu); F[:, nu:, nx:nx + nz] = -K_int
    G[:, :nu], G[:, nu:] = K_fwd, K_int
    integ = fb.integrators_world(n, nu, device)
    loop = fb.connect(cont, integ, feedback=F, inputs=G, reads=ix + iz + list(range(cont.ny, cont.ny + nu)), outputs=iz,
                      input_labels=tuple(f"{s}_ref" for s in z))
    integ.close()
    sr = fb.timeresp.step(loop.world, [(f"{a}_ref", b) for a in z for b in z], t_sim, dt=TS / 4, stride=4)
    loop.world.close()
    return np.einsum("a,iabs->ibs", np.asarray(zref), sr.y.reshape(n, nz, nz, -1))


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    stored = {name: ctl_gains.load_lqr(os.path.join(ctl_gains.DATA_DIR, name + ".h5")) for name in STEPS}
    (e0, e1), (h0, h1) = stored["vh2te"]["bounds"].T
    nE, nH = stored["vh2te"]["K_fbk"].shape[-2:]
    E, H = np.meshgrid(np.linspace(e0, e1, nE), np.linspace(h0, h1, nH), indexing="ij")
    EAS, h = E.ravel(order="F"), H.ravel(order="F")
    n = EAS.size

    w = fb.Cessna172Xv2World(n, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps_schedule(EAS)), scheme="onesided2")
    src = fb.linear_world(w)
    w.close()
    models = {m: fb.c172x_design_model(src, m) for m in ("lon", "lat")}
    src.close()
    print(f"{n} nodes: trimmed {int(lss.success.sum())}; Ts = {TS}")
    worlds = {}
    for name, (zref, t_sim, (lo, hi)) in STEPS.items():
        model, drop, z, qx, qi, r, fwd = DESIGNS[name]
        if (model, drop) not in worlds:
            cont = models[model].world if drop is None else fb.delete_vars_world(models[model].world, drop)
            worlds[model, drop] = (cont, fb.c2d(cont, TS).world)
        cont, P = worlds[model, drop]
        st = stored[name]
        K_fbk, K_fwd, K_int = (np.ascontiguousarray(np.moveaxis(st[k].reshape(st[k].shape[:2] + (-1,), order="F"), -1, 0)) for k in ("K_fbk", "K_fwd", "K_int"))
        u_trim = st["u_trim"].reshape(st["u_trim"].shape[0], -1, order="F").T                      # [N, nu]
        zref = np.array(zref)
        free = fb.dtracker_metrics(P, z, K_fbk, K_fwd, K_int, zref, t_sim)
        held = fb.dtracker_metrics(P, z, K_fbk, K_fwd, K_int, zref, t_sim, bounds=(np.array(lo), np.array(hi)), u_trim=u_trim)
        Cm, D = P.model_cd()
        iz = [P.y_labels.index(s) for s in z]
        direct = bool((D[:, iz] != 0).any())
        print(f"\n{name}: z = {z}, zref = {zref.tolist()}, {t_sim:g} s ({int(round(t_sim / TS))} ticks), nx + nu + nz = {P.nx + P.nu + len(z)}"
              f"{'; D_z != 0: the law reads last tick’s command' if direct else ''}")
        print(" EAS     h   | unbounded: ef                  zp                 up              | bounded: ef                  up              clamped  halted")
        for k in range(n):
            f3 = lambda a: " ".join(f"{v:9.2e}" for v in a)
            f4 = lambda a: " ".join(f"{v:8.4f}" for v in a)
            print(f"{EAS[k]:4.0f} {h[k]:6.0f} | {f3(free.ef[k, 0])} {f4(free.zp[k, 0])} {f4(free.up[k, 0])} | {f3(held.ef[k, 0])} {f4(held.up[k, 0])} "
                  f"{held.clamped[k, 0].tolist()} {held.halted[k, 0].tolist()}")
        if not direct:
            zc = continuous_response(cont, z, K_fbk, K_fwd, K_int, zref, t_sim, device)
            print(f"  the continuous loop with the same gains: ef <= " + " ".join(f"{v:.2e}" for v in np.abs(zref[None] - zc[:, :, -1]).max(axis=0))
                  + "; zp <= " + " ".join(f"{v:.4f}" for v in np.abs(zc).max(axis=(0, 2))) + "; the flown law, unbounded: ef <= "
                  + " ".join(f"{v:.2e}" for v in free.ef[:, 0].max(axis=0)) + "; zp <= " + " ".join(f"{v:.4f}" for v in free.zp[:, 0].max(axis=0)))
        print(f"  status: unbounded {int((free.status != 0).sum())} flagged, bounded {int((held.status != 0).sum())} flagged; the bounded law clamps at "
              f"{int((held.clamped[:, 0] > 0).any(axis=1).sum())} nodes and halts an integrator at {int((held.halted[:, 0] > 0).any(axis=1).sum())}")
        # the gains designed for 50 Hz
        q = [float(qx.get(s, 0.0)) for s in P.x_labels]
        if P.nx + (0 if qi is None else len(qi)) > fb.K["FB_DLQR_NX_MAX"]:
            print("  dlqr_tracker: the augmentation is larger than dlqr takes")
            continue
        Kd_fbk, Kd_fwd, Kd_int, status = fb.dlqr_tracker(P, z, q, np.array(r, dtype=np.float64), qi, forward=fwd, device=device)
        ok = status == 0
        if not ok.any():
            print(f"  dlqr_tracker: not designed (status {sorted(set(status.tolist()))}: {'DIRECT << 8, D_z != 0' if direct else 'see FB_DLQR_*, FB_SURGERY_*'})")
            continue
        rel = lambda a, b: float(np.abs(a[ok] - b[ok]).max() / np.abs(b[ok]).max())
        des = fb.dtracker_metrics(P, z, np.where(ok[:, None, None], Kd_fbk, 0.0), np.where(ok[:, None, None], Kd_fwd, 0.0),
                                  np.where(ok[:, None, None], Kd_int, 0.0), zref, t_sim)
        print(f"  dlqr_tracker at Ts = {TS}: designed {int(ok.sum())} of {n}; against the stored (continuous) gains K_fbk {rel(Kd_fbk, K_fbk):.2e}  "
              f"K_fwd {rel(Kd_fwd, K_fwd):.2e}  K_int {rel(Kd_int, K_int) if np.abs(K_int).max() > 0 else 0.0:.2e}; under the flown law: "
              f"ef <= {des.ef[ok].max():.2e} (stored: {free.ef[ok].max():.2e}), up <= {des.up[ok].max():.4f} (stored: {free.up[ok].max():.4f})")
    for cont, P in worlds.values():
        P.close()
        cont.close()
    for m in models.values():
        try:
            m.world.close()
        except Exception:
            pass


if __name__ == "__main__":
    main()
