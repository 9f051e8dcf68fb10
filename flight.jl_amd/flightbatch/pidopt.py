"""optimize_PID for a batch of linear models on the device (include/flightbatch.h: fb_lss_freqresp, fb_pid_metrics; kernels:
csrc/pid_kernels.hpp; docs/design/linearize.md, "PID loop design on the device").

    reference (FA design/pidopt.jl)                                    here
    PIDData(; k_p, k_i, k_d, τ_f)         FP/control.jl:776-781        PIDData(k_p=, k_i=, k_d=, τ_f=)          (tau_f is an alias)
    Metrics(; Ms, ∫e, ef, ∫u, up)         :8-14                        Metrics(Ms=, ie=, ef=, iu=, up=)         ("∫e", "∫u" are aliases)
    Settings(; t_sim, lower_bounds, ...)  :16-22                       Settings(t_sim=, lower_bounds=, ...)     (+ dt, w, max_iters: ours)
    build_PID(data)                       :31-34                       build_pid(point) -> A, B, C, D
    Metrics(plant, pid, settings), cost   :36-70                       pid_metrics(world, points, u=, y=, settings=, weights=)
    optimize_PID(plant; data_0, ...)      :73-128                      optimize_pid(world, u=, y=, data_0=, settings=, weights=)
    check_results(results, thresholds)    :130-153                     check_results(results, thresholds)

The plant of every call is channel (u, y) of each system of a LinearWorld. What differs from the reference: its step() picks the sample
time and discretises exactly, here the loop is advanced by RK4 with the caller's dt (default: min τ_f / 10; the exact map is flightbatch.c2d; the metrics on it, under the
sampled PID law, are flightbatch.dpid's); its hinfnorm2 finds the exact
peak of the sensitivity and is infinite for an unstable loop, here Ms is the peak over the frequency grid `w` and an unstable loop shows
as DIVERGED; NLopt's GN_DIRECT_L and LN_BOBYQA are not restated: the search is a bounded pattern search, every system of the batch running
its own, all of them in one fb_pid_metrics launch per iteration."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import K as _K, check, lib
from .modeling import _pd, _pi

DIVERGED, SINGULAR, NX_MAX = _K["FB_PID_DIVERGED"], _K["FB_PID_SINGULAR"], _K["FB_PID_NX_MAX"]
M_MAX, NW_MAX, STEPS_MAX = 64, 1024, 200_000
METRIC_NAMES = ("Ms", "ie", "ef", "iu", "up")
_ALIAS = {"∫e": "ie", "∫u": "iu", "tau_f": "τ_f"}


class _Fields:
    """a FieldVector: named fields in a fixed order, the reference's non-ASCII names accepted as keywords and through []"""
    FIELDS: tuple = ()
    DEFAULTS: tuple = ()

    def __init__(self, *args, **kw):
        vals = dict(zip(self.FIELDS, self.DEFAULTS))
        if len(args) == 1 and np.ndim(args[0]) == 1:
            args = tuple(args[0])
        if len(args) > len(self.FIELDS):
            raise TypeError(f"{type(self).__name__} takes {len(self.FIELDS)} values")
        vals.update(zip(self.FIELDS, args))
        for k, v in kw.items():
            k = _ALIAS.get(k, k)
            if k not in self.FIELDS:
                raise TypeError(f"{type(self).__name__} has no field {k!r}")
            vals[k] = v
        missing = [k for k in self.FIELDS if k not in vals]
        if missing:
            raise TypeError(f"{type(self).__name__}: missing {missing}")
        for k in self.FIELDS:
            setattr(self, k, float(vals[k]))

    def __getitem__(self, k):
        return getattr(self, _ALIAS.get(k, k))

    def __array__(self, dtype=None, copy=None):
        return np.array([getattr(self, k) for k in self.FIELDS], dtype=dtype or np.float64)

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{k}={getattr(self, k):g}" for k in self.FIELDS) + ")"


class PIDData(_Fields):
    """one PID point (FP/control.jl:776-781): C(s) = k_p + k_i / s + k_d s / (τ_f s + 1)"""
    FIELDS = ("k_p", "k_i", "k_d", "τ_f")
    DEFAULTS = (1.0, 0.0, 0.1, 0.01)
    tau_f = property(lambda self: self.τ_f)


class Metrics(_Fields):
    """pidopt.jl:8-14: Ms maximum sensitivity, ie (∫e) integrated absolute error, ef absolute final error, iu (∫u) integrated absolute
    control effort, up absolute peak control effort. No defaults, as in the reference; Metrics(np.ones(5)) is its weights' default."""
    FIELDS = METRIC_NAMES


@dataclass
class Settings:
    """pidopt.jl:16-22, and what the device evaluation needs beyond it: dt (None: min τ_f / 10), the frequency grid w in rad/s (None:
    logspace(-2, 3, 321)) and the iteration bound of the pattern search. maxeval and initial_step are NLopt's and are not used."""
    t_sim: float = 5.0
    maxeval: int = 5000
    lower_bounds: PIDData = field(default_factory=lambda: PIDData(k_p=0.0, k_i=0.0, k_d=0.0, τ_f=0.01))
    upper_bounds: PIDData = field(default_factory=lambda: PIDData(k_p=50.0, k_i=50.0, k_d=10.0, τ_f=0.01))
    initial_step: PIDData = field(default_factory=lambda: PIDData(k_p=0.01, k_i=0.01, k_d=0.01, τ_f=0.01))
    dt: float | None = None
    w: np.ndarray | None = None
    max_iters: int = 80


def default_grid() -> np.ndarray:
    return np.logspace(-2.0, 3.0, 321)


@dataclass
class PIDMetricsResult:
    metrics: np.ndarray   # [N, m, 5]  Ms, ie, ef, iu, up
    cost: np.ndarray      # [N, m]
    status: np.ndarray    # [N, m]     0, DIVERGED or SINGULAR


@dataclass
class PIDOptResult:
    data: np.ndarray        # [N, 4]   k_p, k_i, k_d, τ_f
    cost: np.ndarray        # [N]
    metrics: np.ndarray     # [N, 5]
    evals: np.ndarray       # [N]      cost evaluations of this system's search
    iters: np.ndarray       # [N]
    exit_flag: np.ndarray   # [N]      "STEP_TOL_REACHED" or "MAXITER_REACHED"
    status: np.ndarray      # [N]      the status word of the final point


def build_pid(point):
    """(A, B, C, D) of build_PID (pidopt.jl:31-34), states (ξ, η): ξ' = e, η' = (e - η) / τ_f, u = k_p e + k_i ξ + (k_d / τ_f)(e - η)"""
    k_p, k_i, k_d, tf = np.asarray(point, dtype=np.float64)
    if not tf > 0.0:
        raise ValueError(f"build_pid: τ_f = {tf} must be positive")
    return (np.array([[0.0, 0.0], [0.0, -1.0 / tf]]), np.array([[1.0], [1.0 / tf]]), np.array([[k_i, -k_d / tf]]),
            np.array([[k_p + k_d / tf]]))


def _channel(world, u, y):
    def one(v, labels, count, what):
        k = labels.index(v) if isinstance(v, str) else int(v)
        if not 0 <= k < count:
            raise ValueError(f"pidopt: {what} index {k} is outside [0, {count})")
        return k
    return one(u, tuple(world.u_labels), world.nu, "input"), one(y, tuple(world.y_labels), world.ny, "output")


def _grid(w):
    w = default_grid() if w is None else np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 1 or not 1 <= w.size <= NW_MAX:
        raise ValueError(f"pidopt: the frequency grid must be 1-D with 1 to {NW_MAX} entries, got shape {w.shape}")
    if not (np.isfinite(w).all() and (w > 0.0).all()):
        raise ValueError("pidopt: every frequency must be positive and finite")
    return w


def _points(world, points) -> np.ndarray:
    """[N, m, 4] from [N, m, 4], [m, 4] (the same candidates for every system), [4] or PIDData objects"""
    if isinstance(points, PIDData):
        points = [points]
    p = np.asarray([np.asarray(q) for q in points] if isinstance(points, (list, tuple)) else points, dtype=np.float64)
    if p.ndim == 1:
        p = p[None]
    if p.ndim == 2:
        p = np.broadcast_to(p[None], (world.n,) + p.shape)
    if p.ndim != 3 or p.shape[0] != world.n or p.shape[2] != 4:
        raise ValueError(f"pid_metrics: points must be [N = {world.n}, m, 4] (or [m, 4], or PIDData), got {p.shape}")
    if not 1 <= p.shape[1] <= M_MAX:
        raise ValueError(f"pid_metrics: m = {p.shape[1]}, a call takes 1 to {M_MAX} candidates per system")
    if not (p[..., 3] > 0.0).all():
        raise ValueError("pid_metrics: τ_f must be positive at every point")
    return p


def _weights(weights) -> np.ndarray:
    wt = np.ones(5) if weights is None else np.ascontiguousarray(np.asarray(weights), dtype=np.float64)
    if wt.shape != (5,):
        raise ValueError(f"pidopt: weights must be a Metrics or 5 numbers, got shape {wt.shape}")
    if not (np.isfinite(wt).all() and (wt >= 0.0).all() and wt.sum() > 0.0):
        raise ValueError("pidopt: weights must be finite, not negative and not all zero")
    return wt


def _time_grid(settings: Settings, p: np.ndarray):
    dt = float(p[..., 3].min() / 10.0) if settings.dt is None else float(settings.dt)
    t_sim = float(settings.t_sim)
    if not (dt > 0.0 and np.isfinite(dt)):
        raise ValueError(f"pidopt: dt = {dt} must be positive")
    if not (t_sim >= dt and np.isfinite(t_sim)):
        raise ValueError(f"pidopt: t_sim = {t_sim} must be at least dt = {dt}")
    if round(t_sim / dt) > STEPS_MAX:
        raise ValueError(f"pidopt: t_sim / dt = {round(t_sim / dt)} steps, a call takes at most {STEPS_MAX}")
    return t_sim, dt


def freqresp(world, u=0, y=0, w=None) -> np.ndarray:
    """P(jω) = c inv(jωI - A) b + d of channel (u, y) of every system, complex [N, nw], on the device"""
    iu, iy = _channel(world, u, y)
    w = _grid(w)
    re, im = np.empty((w.size, world.n)), np.empty((w.size, world.n))
    check(lib.fb_lss_freqresp(world._h, iu, iy, _pd(w), w.size, _pd(re), _pd(im)))
    return (re + 1j * im).T.copy()


def pid_metrics(world, points, u=0, y=0, settings: Settings | None = None, weights=None) -> PIDMetricsResult:
    """Metrics(plant, build_PID(point), settings) and cost (pidopt.jl:36-70) of every (system, point) pair in one call"""
    settings = settings or Settings()
    iu, iy = _channel(world, u, y)
    p, w, wt = _points(world, points), _grid(settings.w), _weights(weights)
    t_sim, dt = _time_grid(settings, p)
    n, m = p.shape[:2]
    flat = np.ascontiguousarray(p.transpose(2, 1, 0)).reshape(-1)          # [4 x m x N]
    met, cost, status = np.empty((5, m, n)), np.empty((m, n)), np.empty((m, n), dtype=np.int32)
    check(lib.fb_pid_metrics(world._h, iu, iy, _pd(w), w.size, t_sim, dt, _pd(wt), _pd(flat), m, _pd(met), _pd(cost), _pi(status)))
    return PIDMetricsResult(metrics=met.transpose(2, 1, 0).copy(), cost=cost.T.copy(), status=status.T.copy())


def _bounds(settings: Settings):
    lo, hi = np.asarray(settings.lower_bounds, dtype=np.float64), np.asarray(settings.upper_bounds, dtype=np.float64)
    if lo.shape != (4,) or hi.shape != (4,):
        raise ValueError("optimize_pid: lower_bounds and upper_bounds are PIDData (4 numbers)")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError(f"optimize_pid: bounds must be finite with lower <= upper, got {lo} and {hi}")
    if not lo[3] > 0.0:
        raise ValueError(f"optimize_pid: the lower bound of τ_f = {lo[3]} must be positive")
    return lo, hi


def pattern_search(evaluate, n: int, data_0, lower, upper, max_iters: int = 80):
    """The bounded pattern search of optimize_pid, n independent searches advanced together. evaluate(points [n, m, 4]) -> cost [n, m].
    Start: data_0 clipped; step = 0.05 (upper - lower) in every free dimension (lower < upper). An iteration polls ±step and ±step / 4 in
    each free dimension (clipped), moves to the best poll point if it beats the current cost and shrinks the step to a quarter otherwise;
    a search ends when every free step is below 1e-4 (upper - lower), or after max_iters. +Inf never wins.
    Returns x [n, 4], cost [n], evals [n], iters [n], converged [n]."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    span = upper - lower
    free = np.flatnonzero(span > 0.0)
    x = np.clip(np.broadcast_to(np.asarray(data_0, dtype=np.float64), (n, 4)), lower, upper).copy()
    f = np.asarray(evaluate(x[:, None, :]), dtype=np.float64)[:, 0].copy()
    evals, iters = np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    scale = np.full(n, 0.05)                                  # step = scale * span
    active = np.full(n, free.size > 0) & (scale >= 1e-4)
    sign = np.array([1.0, -1.0, 0.25, -0.25])
    for _ in range(int(max_iters)):
        if not active.any():
            break
        poll = np.repeat(x[:, None, :], 4 * free.size, axis=1)
        for k, d in enumerate(free):
            poll[:, 4 * k:4 * k + 4, d] += sign[None, :] * (scale * span[d])[:, None]
        poll = np.clip(poll, lower, upper)
        c = np.asarray(evaluate(poll), dtype=np.float64)
        c = np.where(np.isnan(c), np.inf, c)
        best = c.argmin(axis=1)
        cb = c[np.arange(n), best]
        move = active & (cb < f)
        x[move] = poll[move, best[move]]
        f[move] = cb[move]
        scale[active & ~move] /= 4.0
        evals[active] += 4 * free.size
        iters[active] += 1
        active &= scale >= 1e-4
    return x, f, evals, iters, ~active


def optimize_pid(world, u=0, y=0, data_0=None, settings: Settings | None = None, weights=None) -> PIDOptResult:
    """optimize_PID (pidopt.jl:73-128) for every system of `world`: one pattern search per system (pattern_search), every iteration one
    fb_pid_metrics launch for the whole batch. data_0: a PIDData (or 4 numbers) for the batch, or [N, 4]."""
    settings = settings or Settings()
    lo, hi = _bounds(settings)
    wt = _weights(weights)
    d0 = np.asarray(PIDData() if data_0 is None else data_0, dtype=np.float64)
    if d0.shape not in ((4,), (world.n, 4)):
        raise ValueError(f"optimize_pid: data_0 must be a PIDData or [N = {world.n}, 4], got {d0.shape}")
    if settings.dt is None:
        settings = Settings(**{**settings.__dict__, "dt": float(lo[3]) / 10.0})
    run = lambda pts: pid_metrics(world, pts, u=u, y=y, settings=settings, weights=wt)
    x, f, evals, iters, done = pattern_search(lambda pts: run(pts).cost, world.n, d0, lo, hi, settings.max_iters)
    last = run(x[:, None, :])
    return PIDOptResult(data=x, cost=last.cost[:, 0], metrics=last.metrics[:, 0], evals=evals, iters=iters,
                        exit_flag=np.where(done, "STEP_TOL_REACHED", "MAXITER_REACHED"), status=last.status[:, 0])


def check_results(results, thresholds) -> np.ndarray:
    """check_results (pidopt.jl:130-153) per system: the search ended on its step tolerance and Ms, ie, ef are below the thresholds
    (iu and up are not checked, as in the reference). `results`: a PIDOptResult, or a PIDMetricsResult / metrics array [..., 5]."""
    th = np.asarray(thresholds, dtype=np.float64)
    met = np.asarray(results.metrics if hasattr(results, "metrics") else results, dtype=np.float64)
    ok = (met[..., 0] < th[0]) & (met[..., 1] < th[1]) & (met[..., 2] < th[2])
    if hasattr(results, "exit_flag"):
        ok &= results.exit_flag == "STEP_TOL_REACHED"
    return ok
