"""Step responses and StepInfo of a batch of linear models on the device (include/flightbatch.h: fb_lss_stepinfo; kernels:
csrc/timeresp_kernels.hpp; docs/design/linearize.md, "Step responses on the device").

    reference                                                               here
    step(P[:y, :u], t_sim)            FA design/robot2d/robot2d_design.ipynb     timeresp.step(world, [("u", "y")], t_sim, dt)      world = LinearWorld(lss) / linear_world(...)
    stepinfo(step(...)) |> display                                             print(stepinfo(world, [("u", "y")], t_sim, dt).show(i, 0))

A channel is a pair (iu, iy) of indices into the world's inputs and outputs, or a pair of labels where the world carries them. The response is
that of the deviation model from rest: xdot0, x0, u0 and y0 play no part. Not the reference's: ControlSystems.step picks its own sample time
and discretises exactly; here dt is the caller's (default_dt when None) and the integrator is the classical RK4 of the other steppers."""
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

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0

    def show(self, i: int = 0, j: int = 0) -> str:
        """the reference's nine lines for channel j of system i, in its print format"""
        val = lambda name: float(getattr(self, name)[i, j])
        rows = [("Initial value:", _fmt(val("y0"), "%.3f")), ("Final value:", _fmt(val("yf"), "%.3f")),
                ("Step size:", _fmt(val("stepsize"), "%.3f")), ("Peak:", _fmt(val("peak"), "%.3f")),
                ("Peak time:", _fmt(val("peaktime"), "%.3f") + " s"), ("Overshoot:", _fmt(val("overshoot"), "%5.2f") + " %"),
                ("Undershoot:", _fmt(val("undershoot"), "%5.2f") + " %"), ("Settling time:", _fmt(val("settlingtime"), "%.3f") + " s"),
                ("Rise time:", _fmt(val("risetime"), "%.3f") + " s")]
        return "\n".join("%-19s%s" % r for r in rows)


def _call(world, channels, t_sim, dt, opts, y0, yf, stride, want_y):
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
    return dt, nsteps, y, info, status


def step(world: LinearWorld, channels, t_sim: float, dt: float | None = None, stride: int = 1) -> StepResult:
    """the unit step response of every channel of every system of `world`, every `stride`-th sample and the last one"""
    dt, nsteps, y, _, status = _call(world, channels, t_sim, dt, None, None, None, stride, True)
    ns = y.shape[0]
    t = np.arange(ns, dtype=np.float64) * (stride * dt)
    t[-1] = nsteps * dt
    return StepResult(t=t, y=np.ascontiguousarray(y.transpose(2, 1, 0)), status=status.T.copy())


def stepinfo(world: LinearWorld, channels, t_sim: float, dt: float | None = None, y0=None, yf=None, settling_th: float = 0.02,
             risetime_th=(0.1, 0.9)) -> StepInfo:
    """stepinfo(step(P[:y, :u], t_sim)) of every channel of every system. y0, yf: None, a scalar or [N, m]; NaN entries mean the first / last
    sample."""
    dt, _, _, info, status = _call(world, channels, t_sim, dt, (settling_th, risetime_th[0], risetime_th[1]), y0, yf, 1, False)
    return StepInfo(*[info[k].T.copy() for k in range(9)], status=status.T.copy(), dt=dt)
