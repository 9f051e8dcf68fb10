#!/usr/bin/env python3
"""Where are the modes? Cessna172Sv0(NED) over an EAS x h envelope, every step on the device.

    trim + linearize at every node                      fb.linearize(world, TrimParameters(...))
    the longitudinal and the lateral subsystem          fb.linear_world(world, x=, u=, y=)         device to device: nothing comes home
    the poles of both at every node                     fb.poles(LinearWorld)                      one call per subsystem

Prints the natural frequency and damping ratio of every oscillatory mode (short period, phugoid, Dutch roll), the time constants of the
real ones (roll, spiral, the filters and the engine), and how many nodes have a pole in the right half plane; then the reference's
`dampreport` table of one node. `python examples/modes_envelope.py [nE] [nH] [device]` (default 7 x 4 = 28 nodes)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402

LON = dict(x=("q", "θ", "v_x", "v_z", "α_filt", "ω_eng"), u=("throttle", "elevator"), y=("q", "θ", "α", "EAS"))
LAT = dict(x=("p", "r", "φ", "v_y", "β_filt"), u=("aileron", "rudder"), y=("p", "r", "φ", "β"))


def span(v):
    v = np.asarray(v)
    return f"{np.nanmin(v):8.3f} .. {np.nanmax(v):8.3f}"


def oscillatory(res, names):
    """the complex pairs of every node, fastest first, under the names given; nodes with fewer pairs are left out of that row"""
    up = [lam[lam.imag > 0][::-1] for lam in res.poles]
    for k, name in enumerate(names):
        have = [u[k] for u in up if len(u) > k]
        if have:
            have = np.array(have)
            print(f"  {name:13s} {len(have):4d} nodes   ωn {span(np.abs(have))} rad/s   ζ {span(-np.cos(np.angle(have)))}")


def real_modes(res):
    re = [np.sort(lam[lam.imag == 0].real) for lam in res.poles]
    for k in range(max(len(r) for r in re)):
        have = np.array([r[k] for r in re if len(r) > k])
        with np.errstate(divide="ignore"):
            print(f"  real pole {k}   {len(have):4d} nodes   λ {span(have)} 1/s   τ {span(-1.0 / have)} s")


def main():
    nE = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    nH = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    device = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    E, H = np.meshgrid(np.linspace(30.0, 55.0, nE), np.linspace(50.0, 3050.0, nH), indexing="ij")
    n = E.size
    w = fb.BatchedWorld(n, kinematics="NED", device=device)
    lss = fb.linearize(w, fb.TrimParameters(EAS=E.ravel(), h_e=H.ravel()))
    ok = lss.success & (lss.status == 0)
    print(f"Cessna172Sv0(NED), {nE} x {nH} = {n} nodes, EAS {E.min():.0f} .. {E.max():.0f} m/s, h {H.min():.0f} .. {H.max():.0f} m: "
          f"trimmed and linearised {int(ok.sum())}")
    worlds = {"longitudinal": fb.linear_world(w, **LON), "lateral": fb.linear_world(w, **LAT)}
    w.close()
    unstable = np.zeros(n, dtype=bool)
    first = {}
    for name, lw in worlds.items():
        res = fb.poles(lw)
        lw.close()
        good = ok & (res.status == 0)
        first[name] = res
        print(f"{name}: states {' '.join(lw.x_labels)}; poles found at {int(good.sum())} nodes, QR sweeps {res.iters.min()} .. {res.iters.max()}")
        sel = fb.PolesResult(poles=res.poles[good], iters=res.iters[good], status=res.status[good])
        oscillatory(sel, ("short period", "phugoid") if name == "longitudinal" else ("Dutch roll",))
        real_modes(sel)
        unstable |= good & ~res.stable
    print(f"nodes with a pole in the closed right half plane (unstable): {int(unstable.sum())} of {n}")
    k = int(np.flatnonzero(ok)[0]) if ok.any() else 0
    for name, res in first.items():
        print(f"\n{name} at EAS {E.ravel()[k]:.1f} m/s, h {H.ravel()[k]:.0f} m:")
        print(fb.dampreport(res, k))


if __name__ == "__main__":
    main()
