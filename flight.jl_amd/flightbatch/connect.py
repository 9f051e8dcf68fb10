"""connect / series / feedback for batches of linear models on the device (include/flightbatch.h: fb_lss_connect; kernels:
csrc/connect_kernels.hpp; docs/design/linearize.md, "Closing loops on the device").

    reference                                                                        here
    connect([P, C, ...], connections; w1 = ..., z1 = ...)   FA design/c172/c172x_design.jl:199-216, ...   connect(plant, comp, feedback=F, inputs=G, outputs=...)
    series(1 / s, P)                                        :226-227                                     connect(P, integrator_world(n), ...)
    feedback(P * C)                                         :244-263                                     unity_feedback(P, pid_world(data), u, y)
    the loop u = K_fwd r - K x                              :199-214                                     state_feedback(world, K, K_fwd)

With v = [u_p; u_c] and z = [y_p; y_c] the interconnection is v = F z[reads] + G w; the new world's states are [x_p; x_c], its inputs w and
its outputs z[outputs]. Everything is in deviation coordinates: the new world sits at x = 0, u = 0 with xdot0 = x0 = u0 = y0 = 0. The models
stay on the device from one design verb to the next; only F and G (gains) go up."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .linearization import LinearizedSS
from .lss import LinearWorld, pack_matrix
from .modeling import _pd, _pi

ILL_POSED, NOT_FINITE = _K["FB_CONNECT_ILL_POSED"], _K["FB_CONNECT_NOT_FINITE"]
NV_MAX, NF_MAX, NZ_MAX = _K["FB_CONNECT_NV_MAX"], _K["FB_CONNECT_NF_MAX"], _K["FB_CONNECT_NZ_MAX"]


@dataclass
class ConnectResult:
    world: LinearWorld     # the connected models, an ordinary LinearWorld
    status: np.ndarray     # [N]  0, FB_CONNECT_ILL_POSED or FB_CONNECT_NOT_FINITE (that system's A, B, C, D are NaN)

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0


def _rows(entries, labels, what):
    """indices into z from indices or labels (a label names its first row)"""
    out = []
    for e in entries:
        if isinstance(e, str):
            if e not in labels:
                raise KeyError(f"connect: {e!r} is not an output label of the connected worlds ({what})")
            out.append(labels.index(e))
        else:
            out.append(int(e))
    return np.array(out, dtype=np.int32)


def _gain(M, n, rows, cols, name, verb="connect"):
    """(flat array, per_system) of a gain given as [rows, cols] for the batch or [N, rows, cols] per system; verb: whose message a refusal is"""
    M = np.asarray(M, dtype=np.float64)
    if M.shape == (rows, cols):
        return np.ascontiguousarray(M.reshape(-1, order="F")), 0
    if M.shape == (n, rows, cols):
        return pack_matrix(M), 1
    raise ValueError(f"{verb}: {name} must be [{rows}, {cols}] or [{n}, {rows}, {cols}], got {M.shape}")


def connect(plant: LinearWorld, comp: LinearWorld | None = None, *, feedback, inputs, outputs=None, reads=None, input_labels=None) -> ConnectResult:
    """v = feedback z[reads] + inputs w closed around `plant` (and `comp`), on the device. feedback: F [nv, nf] or [N, nv, nf]; inputs: G
    [nv, nw] or [N, nv, nw]; reads, outputs: rows of z = [y_p; y_c] by index or label (None: every row)."""
    for w, what in ((plant, "plant"), (comp, "compensator")):
        if w is not None and not isinstance(w, LinearWorld):
            raise FlightBatchError(f"connect: the {what} is not a LinearizedSS handle (FB_MODEL_LSS): give it a LinearWorld")
    zl = tuple(plant.y_labels) + (tuple(comp.y_labels) if comp is not None else ())
    nv = plant.nu + (comp.nu if comp is not None else 0)
    jz = _rows(range(len(zl)) if reads is None else reads, zl, "reads")
    iz = None if outputs is None else _rows(outputs, zl, "outputs")
    F, fper = _gain(feedback, plant.n, nv, len(jz), "feedback")
    Gm = np.asarray(inputs, dtype=np.float64)
    nw = Gm.shape[-1] if Gm.ndim in (2, 3) else 0
    G, gper = _gain(Gm, plant.n, nv, nw, "inputs")
    status = np.empty(plant.n, dtype=np.int32)
    h = C.c_void_p()
    check(lib.fb_lss_connect(plant._h, comp._h if comp is not None else None, _pi(jz), len(jz), _pd(F), fper, _pd(G), gper, nw,
                             _pi(iz) if iz is not None else None, len(iz) if iz is not None else 0, _pi(status), C.byref(h)))
    xl = tuple(plant.x_labels) + (tuple(comp.x_labels) if comp is not None else ())
    ul = tuple(input_labels) if input_labels is not None else tuple(f"w{k}" for k in range(nw))
    if len(ul) != nw:
        lib.fb_destroy(h)
        raise ValueError(f"connect: {len(ul)} input labels for {nw} inputs")
    yl = zl if iz is None else tuple(zl[k] for k in iz)
    return ConnectResult(world=LinearWorld(_handle=h, _labels=(xl, ul, yl)), status=status)


def _static_world(n, A, B, Cm, D, xl, ul, yl, device) -> LinearWorld:
    nx, nu, ny = len(xl), len(ul), len(yl)
    z = np.zeros
    return LinearWorld(LinearizedSS(xdot0=z((n, nx)), x0=z((n, nx)), u0=z((n, nu)), y0=z((n, ny)), A=A, B=B, C=Cm, D=D,
                                    x_labels=xl, u_labels=ul, y_labels=yl), device=device)


def integrator_world(n: int, device: int = 0) -> LinearWorld:
    """n copies of 1 / s: ξ' = e, y = ξ"""
    one = np.ones((n, 1, 1))
    return _static_world(n, np.zeros((n, 1, 1)), one, one.copy(), np.zeros((n, 1, 1)), ("ξ",), ("e",), ("ξ",), device)


def pid_world(data, device: int = 0) -> LinearWorld:
    """C(s) = k_p + k_i / s + k_d s / (τ_f s + 1) from PID points [N, 4] (k_p, k_i, k_d, τ_f) in the realisation of fb_pid_metrics:
    A = diag(0, -1 / τ_f), B = (1, 1 / τ_f)', C = (k_i, -k_d / τ_f), D = k_p + k_d / τ_f (states ξ, η)"""
    p = np.asarray(data, dtype=np.float64).reshape(-1, 4)
    n = p.shape[0]
    kp, ki, kd, tf = p.T
    A = np.zeros((n, 2, 2)); A[:, 1, 1] = -1.0 / tf
    B = np.ones((n, 2, 1)); B[:, 1, 0] = 1.0 / tf
    Cm = np.zeros((n, 1, 2)); Cm[:, 0, 0] = ki; Cm[:, 0, 1] = -(kd / tf)
    D = (kp + kd / tf).reshape(n, 1, 1)
    return _static_world(n, A, B, Cm, D, ("ξ", "η"), ("e",), ("u",), device)


def state_feedback(world: LinearWorld, K, K_fwd=None, input_labels=None) -> ConnectResult:
    """u = K_fwd w - K y around a design model whose outputs are its states (C = I): A - B K, B K_fwd, C - D K, D K_fwd. K [nu, nx] or
    [N, nu, nx] (fb_lqr's); K_fwd [nu, nw] or [N, nu, nw] (None: the identity, w takes u's place)."""
    if world.ny != world.nx:
        raise ValueError(f"state_feedback: the world has {world.ny} outputs and {world.nx} states; it takes a design model with C = I")
    G = np.eye(world.nu) if K_fwd is None else K_fwd
    labels = input_labels if input_labels is not None else (world.u_labels if K_fwd is None else None)
    return connect(world, feedback=-np.asarray(K, dtype=np.float64), inputs=G, outputs=None, reads=None, input_labels=labels)


def unity_feedback(plant: LinearWorld, comp: LinearWorld, u=0, y=0, input_labels=None) -> ConnectResult:
    """feedback(plant[y, u] * comp): e = r - y into the one-input, one-output compensator, its output into plant input `u` (the plant's other
    inputs are held at zero). The new world's input is r, its outputs are every row of the plant's y followed by the compensator's output."""
    if comp.nu != 1 or comp.ny != 1:
        raise ValueError("unity_feedback: the compensator must have one input and one output")
    iu = plant.u_labels.index(u) if isinstance(u, str) else int(u)
    iy = plant.y_labels.index(y) if isinstance(y, str) else int(y)
    F = np.zeros((plant.nu + 1, 2))
    F[iu, 1] = 1.0           # u_p[iu] = y_c
    F[plant.nu, 0] = -1.0    # e = r - y
    G = np.zeros((plant.nu + 1, 1)); G[plant.nu, 0] = 1.0
    labels = input_labels if input_labels is not None else (f"{plant.y_labels[iy]}_ref",)
    return connect(plant, comp, feedback=F, inputs=G, reads=[iy, plant.ny], outputs=None, input_labels=labels)
