"""connect / series / feedback for batches of SAMPLED linear models on the device, with unit delays (include/flightbatch.h: fb_lss_dconnect;
kernels: csrc/dconnect_kernels.hpp; docs/design/linearize.md, "Closing sampled loops on the device").

    reference                                                                        here
    connect([P, C, ...], connections; w1 = ..., z1 = ...) on sampled systems          dconnect(plant, comp, feedback=F, inputs=G, delays=..., outputs=...)
    series(C, P) of c2d'd systems                                                     dseries(P, dpid_world(data, Ts), u, y, delay)
    feedback(P * C)                                                                   dunity_feedback(P, dpid_world(data, Ts), u, y, delay)
    the loop u = K_fwd r - K x, computed in one tick and applied in the next          dstate_feedback(world, K, K_fwd, delay=True)

Both worlds are sampled LinearWorlds with the same Ts (c2d(world, Ts).world, dlqr(closed=True).world, LinearWorld(lss, Ts=...), an earlier
dconnect). With v = [u_p; u_c] and z = [y_p; y_c], `delays` names rows of z that are also kept one sample, q_k(t) = z[delays_k](t - 1); the
extended signal vector is [z; q], the new world's states are [x_p; x_c; q]. The interconnection is v = F [z; q][reads] + G w, the outputs are
[z; q][outputs]: a read or an output takes a signal now or one sample late. The delayed copy of a row labelled L is labelled L + "[k-1]",
as a signal and as a state. Everything is in deviation coordinates; the new world is sampled with the plant's Ts and sits at x = 0, u = 0.
A longer delay is a chain of calls. The models stay on the device; only F and G (gains) and the index lists go up."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .connect import ConnectResult, _gain
from .dpid import build_dpid
from .linearization import LinearizedSS
from .lss import LinearWorld
from .modeling import _pd, _pi

ND_MAX = _K["FB_DCONNECT_ND_MAX"]
DELAYED = "[k-1]"


def _rows(entries, labels, what):
    """indices into `labels` from indices or labels (a label names its first row)"""
    out = []
    for e in entries:
        if isinstance(e, str):
            if e not in labels:
                raise KeyError(f"dconnect: {e!r} is not a signal label of the connected worlds ({what})")
            out.append(labels.index(e))
        else:
            out.append(int(e))
    return np.array(out, dtype=np.int32)


def dconnect(plant: LinearWorld, comp: LinearWorld | None = None, *, feedback, inputs, outputs=None, reads=None, delays=(),
             input_labels=None) -> ConnectResult:
    """v = feedback [z; q][reads] + inputs w closed around the sampled `plant` (and `comp`), on the device. delays: rows of z = [y_p; y_c] by
    index or label, q_k(t) = z[delays_k](t - 1); feedback: F [nv, nf] or [N, nv, nf]; inputs: G [nv, nw] or [N, nv, nw]; reads, outputs: rows
    of [z; q] by index or label (None: every row)."""
    for w, what in ((plant, "plant"), (comp, "compensator")):
        if w is not None and not isinstance(w, LinearWorld):
            raise FlightBatchError(f"dconnect: the {what} is not a LinearizedSS handle (FB_MODEL_LSS): give it a LinearWorld")
    zl = tuple(plant.y_labels) + (tuple(comp.y_labels) if comp is not None else ())
    dz = _rows(delays, zl, "delays")
    ql = tuple(f"{zl[k]}{DELAYED}" if 0 <= k < len(zl) else f"q{j}" for j, k in enumerate(dz))   # (an index out of range: the library refuses it)
    zel = zl + ql
    nv = plant.nu + (comp.nu if comp is not None else 0)
    jz = _rows(range(len(zel)) if reads is None else reads, zel, "reads")
    iz = None if outputs is None else _rows(outputs, zel, "outputs")
    F, fper = _gain(feedback, plant.n, nv, len(jz), "feedback", "dconnect")
    Gm = np.asarray(inputs, dtype=np.float64)
    nw = Gm.shape[-1] if Gm.ndim in (2, 3) else 0
    G, gper = _gain(Gm, plant.n, nv, nw, "inputs", "dconnect")
    status = np.empty(plant.n, dtype=np.int32)
    h = C.c_void_p()
    check(lib.fb_lss_dconnect(plant._h, comp._h if comp is not None else None, _pi(dz) if len(dz) else None, len(dz), _pi(jz), len(jz),
                              _pd(F), fper, _pd(G), gper, nw, _pi(iz) if iz is not None else None, len(iz) if iz is not None else 0,
                              _pi(status), C.byref(h)))
    xl = tuple(plant.x_labels) + (tuple(comp.x_labels) if comp is not None else ()) + ql
    ul = tuple(input_labels) if input_labels is not None else tuple(f"w{k}" for k in range(nw))
    if len(ul) != nw:
        lib.fb_destroy(h)
        raise ValueError(f"dconnect: {len(ul)} input labels for {nw} inputs")
    yl = zel if iz is None else tuple(zel[k] for k in iz)
    return ConnectResult(world=LinearWorld(_handle=h, _labels=(xl, ul, yl)), status=status)


def _sampled_world(n, Phi, Gam, Cm, D, xl, ul, yl, Ts, device) -> LinearWorld:
    nx, nu, ny = len(xl), len(ul), len(yl)
    z = np.zeros
    return LinearWorld(LinearizedSS(xdot0=z((n, nx)), x0=z((n, nx)), u0=z((n, nu)), y0=z((n, ny)), A=Phi, B=Gam, C=Cm, D=D,
                                    x_labels=xl, u_labels=ul, y_labels=yl), device=device, Ts=Ts)


def dintegrator_world(n: int, Ts: float, device: int = 0) -> LinearWorld:
    """n copies of the flown backward-Euler integrator Ts z / (z - 1): ξ+ = ξ + Ts e, y = ξ + Ts e"""
    one, ts = np.ones((n, 1, 1)), np.full((n, 1, 1), float(Ts))
    return _sampled_world(n, one, ts, one.copy(), ts.copy(), ("ξ",), ("e",), ("ξ",), Ts, device)


def dpid_world(points, Ts: float, device: int = 0) -> LinearWorld:
    """the sampled PID law from PID points [N, 4] (k_p, k_i, k_d, τ_f >= 0) in build_dpid's realisation (states ξ, η as they stand before a
    tick, input e, output u), as a sampled world"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    blocks = [build_dpid(q, Ts) for q in p]
    Phi, Gam, Cm, D = (np.array([b[k] for b in blocks]) for k in range(4))
    return _sampled_world(p.shape[0], Phi, Gam, Cm, D, ("ξ", "η"), ("e",), ("u",), Ts, device)


def dstate_feedback(world: LinearWorld, K, K_fwd=None, delay: bool = False, input_labels=None) -> ConnectResult:
    """u = K_fwd w - K x around a sampled design model whose outputs are its states (C = I): Phi - Gamma K, Gamma K_fwd. K [nu, nx] or
    [N, nu, nx] (dlqr's); K_fwd [nu, nw] or [N, nu, nw] (None: the identity). delay=True: the control computed from x_k acts at tick k + 1,
    u(t) = K_fwd w(t) - K x(t - 1): the delay is on the reads, the new world has the states [x; x[k-1]] and the outputs of `world`."""
    if world.ny != world.nx:
        raise ValueError(f"dstate_feedback: the world has {world.ny} outputs and {world.nx} states; it takes a design model with C = I")
    G = np.eye(world.nu) if K_fwd is None else K_fwd
    labels = input_labels if input_labels is not None else (world.u_labels if K_fwd is None else None)
    F = -np.asarray(K, dtype=np.float64)
    if not delay:
        return dconnect(world, feedback=F, inputs=G, outputs=None, reads=None, input_labels=labels)
    nz = world.ny
    return dconnect(world, feedback=F, inputs=G, delays=range(nz), reads=range(nz, 2 * nz), outputs=range(nz), input_labels=labels)


def _loop(plant, comp, u, y, delay, verb):
    if comp.nu != 1 or comp.ny != 1:
        raise ValueError(f"{verb}: the compensator must have one input and one output")
    if delay not in (0, 1):
        raise ValueError(f"{verb}: delay = {delay!r}, a call takes 0 or 1 sample (a longer delay is a chain of dconnect calls)")
    iu = plant.u_labels.index(u) if isinstance(u, str) else int(u)
    iy = plant.y_labels.index(y) if isinstance(y, str) else int(y)
    # the compensator's output y_c is row plant.ny of z; delayed, it is row nz = plant.ny + 1 of [z; q]
    return iu, iy, ([plant.ny] if delay else []), plant.ny + (1 if delay else 0)


def dseries(plant: LinearWorld, comp: LinearWorld, u=0, y=0, delay: int = 0, input_labels=None) -> ConnectResult:
    """the open loop plant[y, u] * comp for dmargins: the new world's input is the compensator's, its output into plant input `u` (the plant's
    other inputs are held at zero), now (delay = 0) or one sample late (delay = 1). The outputs are every row of the plant's y followed by
    the compensator's output (`y` is only checked: dmargins and dfreqresp pick the channel)."""
    iu, _, delays, uc = _loop(plant, comp, u, y, delay, "dseries")
    F = np.zeros((plant.nu + 1, 1)); F[iu, 0] = 1.0            # u_p[iu] = y_c, or y_c[k-1]
    G = np.zeros((plant.nu + 1, 1)); G[plant.nu, 0] = 1.0      # the compensator's input is w
    labels = input_labels if input_labels is not None else tuple(comp.u_labels)
    return dconnect(plant, comp, feedback=F, inputs=G, delays=delays, reads=[uc], outputs=range(plant.ny + 1), input_labels=labels)


def dunity_feedback(plant: LinearWorld, comp: LinearWorld, u=0, y=0, delay: int = 0, input_labels=None) -> ConnectResult:
    """feedback(plant[y, u] * comp) in discrete time: e = r - y into the one-input, one-output compensator, its output into plant input `u`
    now (delay = 0) or one sample late (delay = 1: a sample of computational delay). unity_feedback's inputs and outputs: the new world's
    input is r, its outputs are every row of the plant's y followed by the compensator's output."""
    iu, iy, delays, uc = _loop(plant, comp, u, y, delay, "dunity_feedback")
    F = np.zeros((plant.nu + 1, 2))
    F[iu, 1] = 1.0           # u_p[iu] = y_c, or y_c[k-1]
    F[plant.nu, 0] = -1.0    # e = r - y
    G = np.zeros((plant.nu + 1, 1)); G[plant.nu, 0] = 1.0
    labels = input_labels if input_labels is not None else (f"{plant.y_labels[iy]}_ref",)
    return dconnect(plant, comp, feedback=F, inputs=G, delays=delays, reads=[iy, uc], outputs=range(plant.ny + 1), input_labels=labels)
