"""linearize — host side of FP/linearization.jl (LinearizedSS, linearize, subsystem, delete_vars) over the device verbs
fb_linearize / fb_linearize_state (include/flightbatch.h; kernels: csrc/lin_kernels.hpp; docs/design/linearize.md).

    reference                                                        here
    linearize(aircraft, trim_params)    FP/aircraftbase.jl:292-341   linearize(world, TrimParameters(...))
    linearize(robot.vehicle, ip)         FA/robot2d/robot2d.jl:315    linearize(robot2d_world, InitParameters(...) | None)
    linearize(f, h, x0, u0)              FP/linearization.jl:55-111   linearize_state(world)   (the world's current x, u, s, environment)
    subsystem(lss; x, u, y)              FP/linearization.jl:113-132  subsystem(lss, x=..., u=..., y=...)
    delete_vars(lss, s)                  FP/linearization.jl:134-148  delete_vars(lss, names)

A LinearizedSS holds one linear model per aircraft: xdot0, x0 [N, nx], u0 [N, nu], y0 [N, ny], A [N, nx, nx], B [N, nx, nu],
C [N, ny, nx], D [N, ny, nu], with the reference's labels (x_labels, u_labels, y_labels) for the axes."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace
import numpy as np

from ._lib import K, check, lib
from .modeling import BatchedWorld, TrimParameters, TrimState, _pd, _pi

_XS = ("p", "q", "r", "ψ", "θ", "φ", "v_x", "v_y", "v_z", "ϕ", "λ", "h", "α_filt", "β_filt", "ω_eng", "fuel")
_ACT = ("thr_p", "ail_p", "ele_p", "rud_p")
_Y_TAIL = ("f_x", "f_y", "f_z", "α", "β", "EAS", "TAS", "v_N", "v_E", "v_D", "χ", "γ")
# XStateSpace / UStateSpace / YStateSpace of each vehicle, in the reference's field order
LABELS = {
    "FB_MODEL_C172S0": (_XS, ("throttle", "aileron", "elevator", "rudder"),                               # FA/c172/c172s/c172s.jl:269-299
                        _XS + _Y_TAIL + ("c", "throttle_out", "aileron_out", "elevator_out", "rudder_out")),
    "FB_MODEL_C172X2": (_XS + _ACT, ("throttle_cmd", "aileron_cmd", "elevator_cmd", "rudder_cmd"),       # FA/c172/c172x/c172x.jl:332-370
                        _XS[:15] + ("n_eng", "fuel") + _ACT + _Y_TAIL + ("climb_rate", "throttle_cmd", "aileron_cmd", "elevator_cmd", "rudder_cmd")),
    "FB_MODEL_ROBOT2D": (("ω", "v", "θ", "η"), ("m",), ("ω", "v", "θ", "η", "u_m", "τ_m")),             # FA/robot2d/robot2d.jl:233-256
}
SCHEMES = {"forward": "FB_LIN_FORWARD", "onesided2": "FB_LIN_ONESIDED2"}


@dataclass
class LinearizedSS:
    """LinearizedSS (FP/linearization.jl:39-48) for a batch: the leading axis is the aircraft."""
    xdot0: np.ndarray
    x0: np.ndarray
    u0: np.ndarray
    y0: np.ndarray
    A: np.ndarray
    B: np.ndarray
    C: np.ndarray
    D: np.ndarray
    x_labels: tuple
    u_labels: tuple
    y_labels: tuple
    status: np.ndarray | None = None       # OR of the FB_ST_* bits of every evaluation (where the reference would throw)
    success: np.ndarray | None = None      # Cessna: the trim's (fb_linearize only)
    cost: np.ndarray | None = None
    trim_state: np.ndarray | None = None


def _scheme(scheme) -> int:
    if isinstance(scheme, str):
        if scheme not in SCHEMES:
            raise ValueError(f"unknown scheme {scheme!r}: one of {sorted(SCHEMES)}")
        return K[SCHEMES[scheme]]
    return int(scheme)


def dims(world: BatchedWorld):
    nx, nu, ny = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.fb_linearize_dims(world._h, C.byref(nx), C.byref(nu), C.byref(ny)))
    return nx.value, nu.value, ny.value


def _buffers(world):
    nx, nu, ny = dims(world)
    n = world.n
    b = dict(xdot0=np.empty((nx, n)), x0=np.empty((nx, n)), u0=np.empty((nu, n)), y0=np.empty((ny, n)),
             A=np.empty(nx * nx * n), B=np.empty(nx * nu * n), C=np.empty(ny * nx * n), D=np.empty(ny * nu * n),
             status=np.zeros(n, dtype=np.int32))
    ptrs = [_pd(b[k]) for k in ("xdot0", "x0", "u0", "y0", "A", "B", "C", "D")] + [_pi(b["status"])]
    return (nx, nu, ny), b, ptrs


def _result(world, d, b, **extra) -> LinearizedSS:
    nx, nu, ny = d
    n = world.n
    mat = lambda a, r, c: a.reshape(c, r, n).transpose(2, 1, 0).copy()   # [(r + rows c) n + i] -> [i, r, c]
    xl, ul, yl = LABELS[world.MODEL]
    return LinearizedSS(xdot0=b["xdot0"].T.copy(), x0=b["x0"].T.copy(), u0=b["u0"].T.copy(), y0=b["y0"].T.copy(),
                        A=mat(b["A"], nx, nx), B=mat(b["B"], nx, nu), C=mat(b["C"], ny, nx), D=mat(b["D"], ny, nu),
                        x_labels=xl, u_labels=ul, y_labels=yl, status=b["status"], **extra)


def linearize(world: BatchedWorld, params=None, trim_state=None, scheme="forward") -> LinearizedSS:
    """linearize(vehicle, trim_params) (FP/aircraftbase.jl:292-334): trim in still air at the ISA sea level (whatever the world's wind,
    sea level and terrain), then A, B, C, D about the trim; the world is left trimmed, as f_init would leave it after that trim.
    Cessna: params = TrimParameters or a packed [FB_NTP, n] array. Robot2D (FA/robot2d/robot2d.jl:315-341): InitParameters, a packed
    [3, n] array, or None for the defaults."""
    d, b, ptrs = _buffers(world)
    n = world.n
    if world.MODEL == "FB_MODEL_ROBOT2D":
        ip = None if params is None else np.ascontiguousarray(params.pack(n) if hasattr(params, "pack") else params, dtype=np.float64).reshape(3, n)
        check(lib.fb_linearize(world._h, None if ip is None else _pd(ip), None, None, None, _scheme(scheme), *ptrs))
        world.t = 0.0
        return _result(world, d, b)
    if params is None:
        raise TypeError("linearize: a Cessna needs trim parameters")
    tp = np.ascontiguousarray(params.pack(n) if isinstance(params, TrimParameters) else params, dtype=np.float64).reshape(K["FB_NTP"], n)
    ts = TrimState(n) if trim_state is None else np.ascontiguousarray(trim_state, dtype=np.float64).reshape(K["FB_NTS"], n).copy()
    ok = np.zeros(n, dtype=np.int32)
    cost = np.zeros(n)
    check(lib.fb_linearize(world._h, _pd(tp), _pd(ts), _pi(ok), _pd(cost), _scheme(scheme), *ptrs))
    world.trim_state, world.trim_success, world.trim_cost = ts, ok.astype(bool), cost
    world.t = 0.0
    return _result(world, d, b, success=ok.astype(bool), cost=cost, trim_state=ts)


def linearize_state(world: BatchedWorld, scheme="forward") -> LinearizedSS:
    """linearize(f, h, x0, u0) (FP/linearization.jl:55-111) at the world's current x, u, s and environment; changes nothing."""
    d, b, ptrs = _buffers(world)
    check(lib.fb_linearize_state(world._h, _scheme(scheme), *ptrs))
    return _result(world, d, b)


def _index(labels, names, what):
    out = []
    for s in names:
        if s not in labels:
            raise KeyError(f"{s!r} is not a {what} label")
        out.append(labels.index(s))
    return out


def subsystem(lss: LinearizedSS, x=None, u=None, y=None) -> LinearizedSS:
    """subsystem(lss; x, u, y) (FP/linearization.jl:113-132): the rows / columns of the named variables, in the order given"""
    xl = tuple(lss.x_labels if x is None else x)
    ul = tuple(lss.u_labels if u is None else u)
    yl = tuple(lss.y_labels if y is None else y)
    ix, iu, iy = _index(lss.x_labels, xl, "state"), _index(lss.u_labels, ul, "input"), _index(lss.y_labels, yl, "output")
    return replace(lss, xdot0=lss.xdot0[:, ix], x0=lss.x0[:, ix], u0=lss.u0[:, iu], y0=lss.y0[:, iy],
                   A=lss.A[:, ix][:, :, ix], B=lss.B[:, ix][:, :, iu], C=lss.C[:, iy][:, :, ix], D=lss.D[:, iy][:, :, iu],
                   x_labels=xl, u_labels=ul, y_labels=yl)


def delete_vars(lss: LinearizedSS, names) -> LinearizedSS:
    """delete_vars(lss, s) (FP/linearization.jl:134-148): every named variable leaves each axis it appears on"""
    names = [names] if isinstance(names, str) else list(names)
    keep = lambda labels: [s for s in labels if s not in names]
    return subsystem(lss, x=keep(lss.x_labels), u=keep(lss.u_labels), y=keep(lss.y_labels))
