"""Step responses and StepInfo of a batch of linear models on the device (include/flightbatch.h: fb_lss_stepinfo; kernels:
csrc/timeresp_kernels.hpp; docs/design/linearize.md, "Step responses on the device").

    reference                                                               here
    step(P[:y, :u], t_sim)            FA design/robot2d/robot2d_design.ipynb     timeresp.step(world, [("u", "y")], t_sim, dt)      world = LinearWorld(lss) / linear_world(...)
    stepinfo(step(...)) |> display                                             print(stepinfo(world, [("u", "y")], t_sim, dt).show(i, 0))

A channel is a pair (iu, iy) of indices into the world's inputs and outputs, or a pair of labels where the world carries them. The response is
that of the deviation model from rest: xdot0, x0, u0 and y0 play no part. Not the reference's: ControlSystems.step picks its own sample time
and discretises exactly; here dt is the caller's (default_dt when None) and the integrator is the classical RK4 of the other steppers
(method="rk4", the default) or, with method="zoh", the exact zero-order-hold map of flightbatch.c2d at that dt, whose samples are exact.

    lsim(sys, u, t)                   FA demos/c172_demos.jl:135, 186            timeresp.lsim(world, u, t)    (zero-order hold, existing verbs only)"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .lss import LinearWorld
from .modeling import _pd, _pi

DIVERGED, FLAT, NX_MAX = _K["FB_STEPINFO_DIVERGED"], _K["FB_STEPINFO_FLAT"], _K["FB_STEPINFO_NX_MAX"]
FIELDS = ("y0", "yf", "stepsize", "peak", "peaktime", "overshoot", "undershoot", "settlingtime", "risetime")   # the rows of info


def samples(nsteps: int, stride: int = 1) -> int:
    """rows of the sample buffer: ceil(nsteps / stride) + 1 (fb_lss_stepinfo_samples)"""
    ns = int(lib.fb_lss_stepinfo_samples(int(nsteps), int(stride)))
    if ns < 0:
        raise FlightBatchError(f"fb_lss_stepinfo_samples: nsteps = {nsteps} and stride = {stride} must both be at least 1")
    return ns


def default_dt(world: LinearWorld) -> float:
    """1 / (12 max|pole|) over the batch, rounded to two significant digits (modelled on ControlSystems' default, not claimed equal to it)"""
    from .poles import poles
    res = poles(world)
    wn = res.wn[res.status == 0]
    top = float(wn.max()) if wn.size else 0.0
    if not (top > 0.0) or not np.isfinite(top):
        raise FlightBatchError("default_dt: the batch has no finite non-zero pole to take a sample time from: pass dt")
    return float("%.1e" % (1.0 / (12.0 * top)))


def _channels(world: LinearWorld, channels):
    iu, iy = [], []
    for ch in channels:
        u, y = ch
        if isinstance(u, str):
            if u not in world.u_labels:
                raise KeyError(f"{u!r} is not an input label")
            u = world.u_labels.index(u)
        if isinstance(y, str):
            if y not in world.y_labels:
                raise KeyError(f"{y!r} is not an output label")
            y = world.y_labels.index(y)
        iu.append(int(u)); iy.append(int(y))
    return np.array(iu, dtype=np.int32), np.array(iy, dtype=np.int32)


def _fmt(v: float, spec: str) -> str:
    return "NaN".rjust(5 if spec.startswith("%5") else 0) if np.isnan(v) else spec % v


@dataclass
class StepResult:
    t: np.ndarray        # [ns]        sample times: s stride dt, the last one N dt
    y: np.ndarray        # [N, m, ns]  the response of channel j of system i
    status: np.ndarray   # [N, m]      0, or FB_STEPINFO_DIVERGED / FB_STEPINFO_FLAT
    c2d_status: np.ndarray | None = None   # [N] method="zoh" on a continuous world: the discretisation's status words (FB_C2D_*), else None


@dataclass
class StepInfo:
    y0: np.ndarray            # every field [N, m]
    yf: np.ndarray
    stepsize: np.ndarray
    peak: np.ndarray
    peaktime: np.ndarray
    overshoot: np.ndarray     # %
    undershoot: np.ndarray    # %
    settlingtime: np.ndarray
    risetime: np.ndarray
    status: np.ndarray        # [N, m] 0, FB_STEPINFO_DIVERGED (every field NaN) or FB_STEPINFO_FLAT (the ratios and times NaN)
    dt: float
    c2d_status: np.ndarray | None = None   # [N] method="zoh" on a continuous world: the discretisation's status words (FB_C2D_*), else None

    @property
    def ok(self) -> np.ndarray:
        return (self.status == 0) if self.c2d_status is None else (self.status == 0) & (self.c2d_status == 0)[:, None]

    def show(self, i: int = 0, j: int = 0) -> str:
        """the reference's nine lines for channel j of system i, in its print format"""
        val = lambda name: float(getattr(self, name)[i, j])
        rows = [("Initial value:", _fmt(val("y0"), "%.3f")), ("Final value:", _fmt(val("yf"), "%.3f")),
                ("Step size:", _fmt(val("stepsize"), "%.3f")), ("Peak:", _fmt(val("peak"), "%.3f")),
                ("Peak time:", _fmt(val("peaktime"), "%.3f") + " s"), ("Overshoot:", _fmt(val("overshoot"), "%5.2f") + " %"),
                ("Undershoot:", _fmt(val("undershoot"), "%5.2f") + " %"), ("Settling time:", _fmt(val("settlingtime"), "%.3f") + " s"),
                ("Rise time:", _fmt(val("risetime"), "%.3f") + " s")]
        return "\n".join("%-19s%s" % r for r in rows)


def _call(world, channels, t_sim, dt, opts, y0, yf, stride, want_y, method="rk4"):
    """(dt, nsteps, y, info, status, c2d_status) of one fb_lss_stepinfo call; method="zoh" on a continuous world discretises it at dt first
    (a temporary sampled world, destroyed afterwards); a sampled world runs its own map at its own Ts"""
    if method not in ("rk4", "zoh"):
        raise ValueError('timeresp: method is "rk4" or "zoh"')
    Ts = world.Ts if isinstance(world, LinearWorld) else 0.0      # (any other world: the library refuses it by name below)
    if Ts > 0.0:
        dt = Ts if dt is None else float(dt)
    elif method == "zoh":
        from .c2d import c2d
        dt = default_dt(world) if dt is None else float(dt)
        res = c2d(world, dt)
        try:
            return _call(res.world, channels, t_sim, dt, opts, y0, yf, stride, want_y)[:5] + (res.status,)
        finally:
            res.world.close()
    iu, iy = _channels(world, channels)
    m, n = len(iu), world.n
    dt = default_dt(world) if dt is None else float(dt)
    pack = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, m)).T)
    y0p, yfp = pack(y0), pack(yf)
    nsteps = int(round(float(t_sim) / dt)) if dt > 0 and np.isfinite(dt) and np.isfinite(t_sim) else 0
    y = np.empty((samples(nsteps, stride), m, n)) if want_y and 1 <= nsteps <= 200000 and stride >= 1 and 1 <= m <= 64 else None
    info, status = np.empty((9, m, n)), np.empty((m, n), dtype=np.int32)
    o = None if opts is None else np.array(opts, dtype=np.float64)
    check(lib.fb_lss_stepinfo(world._h, _pi(iu), _pi(iy), m, float(t_sim), dt, None if o is None else _pd(o),
                              None if y0p is None else _pd(y0p), None if yfp is None else _pd(yfp), int(stride),
                              None if y is None else _pd(y), _pd(info), _pi(status)))
    return dt, nsteps, y, info, status, None


def step(world: LinearWorld, channels, t_sim: float, dt: float | None = None, stride: int = 1, method: str = "rk4") -> StepResult:
    """the unit step response of every channel of every system of `world`, every `stride`-th sample and the last one. method: "rk4", or
    "zoh" for the exact samples of the zero-order-hold map (c2d at dt); a sampled world is sampled at its own Ts either way."""
    dt, nsteps, y, _, status, c2d_status = _call(world, channels, t_sim, dt, None, None, None, stride, True, method)
    ns = y.shape[0]
    t = np.arange(ns, dtype=np.float64) * (stride * dt)
    t[-1] = nsteps * dt
    return StepResult(t=t, y=np.ascontiguousarray(y.transpose(2, 1, 0)), status=status.T.copy(), c2d_status=c2d_status)


def stepinfo(world: LinearWorld, channels, t_sim: float, dt: float | None = None, y0=None, yf=None, settling_th: float = 0.02,
             risetime_th=(0.1, 0.9), method: str = "rk4") -> StepInfo:
    """stepinfo(step(P[:y, :u], t_sim)) of every channel of every system. y0, yf: None, a scalar or [N, m]; NaN entries mean the first / last
    sample. method: as step's."""
    dt, _, _, info, status, c2d_status = _call(world, channels, t_sim, dt, (settling_th, risetime_th[0], risetime_th[1]), y0, yf, 1, False, method)
    return StepInfo(*[info[k].T.copy() for k in range(9)], status=status.T.copy(), dt=dt, c2d_status=c2d_status)


def lsim(world: LinearWorld, u, t, x0=None):
    """(y [nt, ny, N], x [nt, nx, N]) of every system of `world` under the input u held over each interval of the uniform time vector t
    (zero-order hold, exact at the samples): x_{k+1} = x0 + Phi (x_k - x0) + Gamma (u_k - u0) + delta and y_k = y0 + C (x_k - x0) +
    D (u_k - u0) with the u of sample k. u: [nt, nu] for the batch or [nt, nu, N] per system ([nt] where nu == 1), the inputs themselves
    (not deviations from u0). x0: the initial state [nx] or [nx, N]; None: the world's current state (a world fresh from linear_world or
    c2d sits at its linearisation point). A continuous world is discretised at t[1] - t[0] into a temporary world, which is destroyed
    afterwards, and is itself left untouched; a sampled world must have that Ts, and is left at the last sample with its log off.
    Existing verbs only: runs of equal consecutive inputs advance in one step() with the device log, and the sample at a change of input is
    recorded after the new input is set."""
    if not isinstance(world, LinearWorld):
        raise FlightBatchError("lsim: the world is not a LinearizedSS handle (FB_MODEL_LSS): give it a LinearWorld")
    t = np.asarray(t, dtype=np.float64)
    nt = t.size
    if t.ndim != 1 or nt < 2:
        raise ValueError("lsim: t is a vector of at least two instants")
    dt = float(t[1] - t[0])
    if not (dt > 0.0) or not np.allclose(np.diff(t), dt, rtol=1e-9, atol=0.0):
        raise ValueError("lsim: t must be uniform and increasing")
    n, nx, nu, ny = world.n, world.nx, world.nu, world.ny
    u = np.asarray(u, dtype=np.float64)
    if u.ndim == 1 and nu == 1:
        u = u[:, None]
    if u.ndim == 2:
        u = np.broadcast_to(u[:, :, None], u.shape + (n,))
    if u.shape != (nt, nu, n):
        raise ValueError(f"lsim: u is [nt, nu] or [nt, nu, N] = [{nt}, {nu}, {n}], got {list(u.shape)}")
    start = world.x if x0 is None else np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(nx, -1), (nx, n))
    Ts = world.Ts
    own = None
    if Ts > 0.0:
        if abs(Ts - dt) > 1e-9 * Ts:
            raise FlightBatchError(f"lsim: the world is sampled at Ts = {Ts!r}, the time vector steps by {dt!r}")
        w = world
    else:
        from .c2d import c2d
        own = c2d(world, dt)
        w = own.world
        if not own.ok.all():
            bad = np.flatnonzero(~own.ok)
            w.close()
            raise FlightBatchError(f"lsim: c2d flagged systems {bad.tolist()} (status {own.status[bad].tolist()})")
    try:
        change = np.flatnonzero((u[1:] != u[:-1]).any(axis=(1, 2))) + 1          # the samples that begin a run
        starts = np.concatenate([[0], change])
        w.set_state(np.ascontiguousarray(start))
        w.log_configure(1, nt + len(starts), y=range(ny), x=range(nx))
        at = np.empty(nt, dtype=np.int64)      # where sample k lies in the log: its last record
        pos = 0
        for j, k in enumerate(starts):
            end = int(starts[j + 1]) if j + 1 < len(starts) else nt - 1          # the run's input takes the state to sample `end`
            w.u = np.ascontiguousarray(u[k])
            check(lib.fb_log_record(w._h))                                     # sample k with the new input (f_ode, then the rows)
            at[k] = pos
            steps = end - int(k)
            if steps > 0:
                w.step(steps)
                at[k + 1:end + 1] = pos + 1 + np.arange(steps)
            pos += 1 + steps
        _, data = w.log_read()
        w.log_configure(0, 0)
    finally:
        if own is not None:
            w.close()
    data = data[at]
    return np.ascontiguousarray(data[:, :ny]), np.ascontiguousarray(data[:, ny:])
