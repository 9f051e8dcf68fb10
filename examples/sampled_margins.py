#!/usr/bin/env python3
"""What the sample time and a sample of computational delay do to the margins of a designed loop, on the device: the position loop of
the reference's Robot2D design notebook (lib/FlightApps/design/robot2d/robot2d_design.ipynb; examples/loop_margins.py shows it in
continuous time at GM 3.673, PM 60.53° for k_p = 1), run the way the reference runs its controllers: in f_periodic! at a fixed rate, on
gains designed in continuous time.

    the velocity loop P_v (LQR tracker around the linearised vehicle)      as in examples/loop_margins.py                          on the device
    marginplot(series(C_η2v, P_v2η)), a batch of k_p                       fb.margins(P_v, u="v_ref", y="η", gain=k_p)             on the device
    c2d(P_v, Ts), one world per Ts                                         fb.c2d(P_v, Ts).world                                   on the device
    margin(k_p c2d(P_v, Ts))                                               fb.dmargins(world, u="v_ref", y="η", gain=k_p)          on the device
    ... with the command applied one sample late, z⁻¹                      Φ, Γ, C, D of the c2d world, the delay state appended on the host,
                                                                           handed back through fb.LinearWorld(lss, Ts=Ts): Φ has an eigenvalue
                                                                           at 0, so no c2d makes this world
    is the closed position loop stable?                                    fb.dpoles of Φ - k_p γ c, made the same way

Beside the numbers, the rule of thumb: half a sample of hold and each half sample of delay cost ω_gc Ts / 2 of phase margin.
`python examples/sampled_margins.py [device]`"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
import flightbatch as fb  # noqa: E402

K_P = np.array([0.3, 0.6, 1.2])        # the notebook's C_η2v is 0.6
TS = (0.02, 0.1, 0.3, 0.6)             # the reference's controllers run at 0.02


def velocity_loop(n, device):
    w = fb.Robot2DWorld(n, device=device)
    fb.linearize(w, None, scheme="forward")
    plant = fb.linear_world(w)
    w.close()
    red = fb.subsystem_world(plant, x=["ω", "v", "θ"])
    K_fbk, K_fwd, K_int, status = fb.lqr_tracker(red, ["v"], [1e-3, 1e-2, 0.0], np.array([[1e-1]]), [5e-2], device=device)
    red.close()
    assert (status == 0).all(), status
    K_x, k_fwd, k_int = K_fbk[0, 0], float(K_fwd[0, 0, 0]), float(K_int[0, 0, 0])
    integ = fb.integrator_world(n, device=device)
    F = np.array([[-K_x[0], -K_x[1], -K_x[2], -1.0], [0.0, k_int, 0.0, 0.0]])
    vel = fb.connect(plant, integ, feedback=F, inputs=np.array([[k_fwd], [-k_int]]), reads=["ω", "v", "θ", "ξ"], input_labels=("v_ref",))
    assert vel.ok.all()
    plant.close(); integ.close()
    return vel.world


def channel(world):
    """(Φ [n, nx, nx], γ [n, nx], c [n, nx], d [n]) of v_ref -> η as the device holds them"""
    Phi, Gam = world.model()
    Cm, D = world.model_cd()
    iu, iy = world.u_labels.index("v_ref"), world.y_labels.index("η")
    return Phi, Gam[:, :, iu], Cm[:, iy, :], D[:, iy, iu]


def given(Phi, gam, c, d, Ts, device):
    """a sampled single-channel world from its matrices"""
    n, nx = gam.shape
    z = lambda *shape: np.zeros((n,) + shape)
    lss = fb.LinearizedSS(xdot0=z(nx), x0=z(nx), u0=z(1), y0=z(1), A=Phi, B=gam[:, :, None], C=c[:, None, :], D=d.reshape(n, 1, 1),
                          x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=("v_ref",), y_labels=("η",))
    return fb.LinearWorld(lss, device=device, Ts=Ts)


def delayed(Phi, gam, c, d):
    """the channel with its input one sample late: the state gains the last command"""
    n, nx = gam.shape
    P, g, cc = np.zeros((n, nx + 1, nx + 1)), np.zeros((n, nx + 1)), np.zeros((n, nx + 1))
    P[:, :nx, :nx], P[:, :nx, nx], g[:, nx] = Phi, gam, 1.0
    cc[:, :nx], cc[:, nx] = c, d
    return P, g, cc, np.zeros(n)


def closed_stable(Phi, gam, c, d, Ts, device):
    """whether Φ - k γ c / (1 + k d) has every pole inside the unit circle, per loop gain"""
    k = K_P / (1.0 + K_P * d)
    cl = given(Phi - k[:, None, None] * gam[:, :, None] * c[:, None, :], gam, c, d, Ts, device)
    res = fb.dpoles(cl)
    cl.close()
    return res.stable, np.abs(res.poles).max(axis=1)


def main():
    device = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    vel = velocity_loop(K_P.size, device)
    cont = fb.margins(vel, u="v_ref", y="η", gain=K_P)
    print("the position loop η <- v_ref, k_p = " + ", ".join(f"{k:g}" for k in K_P))
    print("continuous:        " + "   ".join(f"GM {g:6.3f} PM {p:6.2f}° at {w:.4f} rad/s" for g, p, w in zip(cont.gm, cont.pm, cont.wgc)))
    for Ts in TS:
        zoh = fb.c2d(vel, Ts).world
        m = fb.dmargins(zoh, u="v_ref", y="η", gain=K_P)
        blocks = channel(zoh)
        zoh.close()
        late = given(*delayed(*blocks), Ts, device)
        md = fb.dmargins(late, gain=K_P)
        late.close()
        st, rho = closed_stable(*blocks, Ts, device)
        std, rhod = closed_stable(*delayed(*blocks), Ts, device)
        thumb = np.degrees(cont.wgc * Ts / 2.0)
        print(f"Ts = {Ts:g} s (Nyquist {np.pi / Ts:.1f} rad/s)")
        print("  zero-order hold: " + "   ".join(f"GM {g:6.3f} PM {p:6.2f}° (thumb {c - t:6.2f}°)" for g, p, c, t in zip(m.gm, m.pm, cont.pm, thumb))
              + "   closed loop " + ", ".join(f"{'stable' if s else 'UNSTABLE'} |z| {r:.4f}" for s, r in zip(st, rho)))
        print("  + a sample delay:" + "   ".join(f"GM {g:6.3f} PM {p:6.2f}° (thumb {c - 3 * t:6.2f}°)" for g, p, c, t in zip(md.gm, md.pm, cont.pm, thumb))
              + "   closed loop " + ", ".join(f"{'stable' if s else 'UNSTABLE'} |z| {r:.4f}" for s, r in zip(std, rhod)))
        assert m.ok.all() and md.ok.all()
    vel.close()


if __name__ == "__main__":
    main()
