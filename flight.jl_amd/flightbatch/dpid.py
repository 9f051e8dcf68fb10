"""Discrete PID design on the device: optimize_PID's metrics under the sampled law the stepper flies, for a batch of sampled models
(include/flightbatch.h: fb_lss_dpid_metrics; kernels: csrc/dpid_kernels.hpp; docs/design/linearize.md, "Discrete PID design on the device").

    reference                                                          here
    f_periodic! of PID                    FP/control.jl:431-471        the law of dpid_metrics, per (system, point) pair
    Metrics(plant, pid, settings), cost   FA design/pidopt.jl:36-70    dpid_metrics(world, points, u=, y=, settings=, weights=, bounds=, w=)
    optimize_PID(plant; data_0, ...)      :73-128                      optimize_dpid(world, u=, y=, data_0=, settings=, weights=, bounds=, w=)
    build_PID(data)                       :31-34                       build_dpid(point, Ts) -> Phi_c, Gamma_c, C_c, D_c

The world is a sampled LinearWorld (c2d(world, Ts).world, or LinearWorld(lss, Ts=...)); the plant is channel (u, y) of each system. Per tick
of Ts: a backward-Euler integrator, a backward-Euler filtered derivative (α = 1 / (τ_f + Ts); τ_f = 0 is the plain backward difference), an
optional output clamp and an integrator that halts while the output is clamped and the error pushes further into the bound. The response
is stepped by the exact map for N = round(t_sim / Ts) ticks. Ms is the sensitivity peak of the LINEAR law over the grid `w` (rad/s, at most
π/Ts; default default_dgrid(Ts)): the bounds play no part in it. PIDData, Metrics, Settings, check_results and pattern_search are
flightbatch.pidopt's; Settings.dt is not used here (the tick is the world's Ts)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, check, lib
from .dfreq import _dgrid, _sampled
from .modeling import _pd, _pi
from .pidopt import M_MAX, STEPS_MAX, PIDData, PIDOptResult, Settings, _channel, _weights, pattern_search

DIVERGED, SINGULAR, DIRECT, NX_MAX = (_K[k] for k in ("FB_DPID_DIVERGED", "FB_DPID_SINGULAR", "FB_DPID_DIRECT", "FB_DPID_NX_MAX"))


@dataclass
class DPIDMetricsResult:
    metrics: np.ndarray   # [N, m, 5]  Ms, ie, ef, iu, up
    cost: np.ndarray      # [N, m]
    status: np.ndarray    # [N, m]     0, DIVERGED, SINGULAR or DIRECT
    counts: np.ndarray    # [N, m, 2]  ticks with the output clamped, ticks with the integrator halted (of k = 0 .. N)


def build_dpid(point, Ts):
    """(Phi_c, Gamma_c, C_c, D_c) of the unbounded law from e to u, states (ξ, η) as they stand before a tick:
    ξ+ = ξ + Ts k_i e, η+ = α τ_f η + Ts α k_d e, u = (k_p + Ts k_i + α k_d) e + ξ - α η; its transfer function is
    C(z) = k_p + k_i Ts z / (z - 1) + k_d α (z - 1) / (z - α τ_f). LinearWorld(lss, Ts=Ts) accepts it as a sampled model."""
    k_p, k_i, k_d, tf = np.asarray(point, dtype=np.float64)
    Ts = float(Ts)
    if not (Ts > 0.0 and np.isfinite(Ts)):
        raise ValueError(f"build_dpid: Ts = {Ts} must be positive and finite")
    if not (tf >= 0.0 and np.isfinite(tf)):
        raise ValueError(f"build_dpid: τ_f = {tf} must be finite and not negative")
    al = 1.0 / (tf + Ts)
    return (np.array([[1.0, 0.0], [0.0, al * tf]]), np.array([[Ts * k_i], [Ts * al * k_d]]), np.array([[1.0, -al]]),
            np.array([[k_p + Ts * k_i + al * k_d]]))


def dpid_response(point, Ts, w) -> np.ndarray:
    """C(e^(jωTs)) of the law on the frequencies w (rad/s): complex [nw]"""
    k_p, k_i, k_d, tf = np.asarray(point, dtype=np.float64)
    z = np.exp(1j * np.asarray(w, dtype=np.float64) * Ts)
    al = 1.0 / (tf + Ts)
    return k_p + k_i * Ts * z / (z - 1.0) + k_d * al * (z - 1.0) / (z - al * tf)


def _dpoints(world, points) -> np.ndarray:
    """[N, m, 4] from [N, m, 4], [m, 4] (the same candidates for every system), [4] or PIDData objects; τ_f >= 0"""
    if isinstance(points, PIDData):
        points = [points]
    p = np.asarray([np.asarray(q) for q in points] if isinstance(points, (list, tuple)) else points, dtype=np.float64)
    if p.ndim == 1:
        p = p[None]
    if p.ndim == 2:
        p = np.broadcast_to(p[None], (world.n,) + p.shape)
    if p.ndim != 3 or p.shape[0] != world.n or p.shape[2] != 4:
        raise ValueError(f"dpid_metrics: points must be [N = {world.n}, m, 4] (or [m, 4], or PIDData), got {p.shape}")
    if not 1 <= p.shape[1] <= M_MAX:
        raise ValueError(f"dpid_metrics: m = {p.shape[1]}, a call takes 1 to {M_MAX} candidates per system")
    if not (np.isfinite(p[..., 3]).all() and (p[..., 3] >= 0.0).all()):
        raise ValueError("dpid_metrics: τ_f must be finite and not negative at every point")
    return p


def _out_bounds(bounds, n, m):
    """None, or (lo, hi) with each side a number, [N] or [N, m]: flat [2 x m x N]"""
    if bounds is None:
        return None
    if len(bounds) != 2:
        raise ValueError("dpid_metrics: bounds must be None or a pair (lo, hi)")

    def side(v):
        v = np.asarray(v, dtype=np.float64)
        return np.broadcast_to(v[:, None] if v.ndim == 1 else v, (n, m))
    lo, hi = side(bounds[0]), side(bounds[1])
    if np.isnan(lo).any() or np.isnan(hi).any() or not (lo < hi).all():
        raise ValueError("dpid_metrics: the output bounds must satisfy lo < hi (either may be infinite)")
    return np.ascontiguousarray(np.stack([lo.T, hi.T])).reshape(-1)


def _ticks(world, settings) -> float:
    Ts, t_sim = float(world.Ts), float(settings.t_sim)
    if Ts > 0.0 and not (np.isfinite(t_sim) and 1 <= round(t_sim / Ts) <= STEPS_MAX):
        raise ValueError(f"dpid_metrics: t_sim = {t_sim} at Ts = {Ts} gives {t_sim / Ts:g} ticks, a call takes 1 to {STEPS_MAX}")
    return t_sim


def dpid_metrics(world, points, u=0, y=0, settings: Settings | None = None, weights=None, bounds=None, w=None) -> DPIDMetricsResult:
    """the five metrics, the cost, the status word and the clamp / halt counts of every (system, point) pair of a sampled LinearWorld under
    the sampled PID law, in one call. bounds: None or (lo, hi), each a number, [N] or [N, m]; w: the grid (default: settings.w, then
    default_dgrid(world.Ts))"""
    settings = settings or Settings()
    iu, iy = _channel(world, u, y)
    p, wt = _dpoints(world, points), _weights(weights)
    n, m = p.shape[:2]
    bnd = _out_bounds(bounds, n, m)
    _sampled(world, "dpid_metrics")
    t_sim = _ticks(world, settings)
    w = _dgrid(world, settings.w if w is None else w, "dpid_metrics", 1)
    flat = np.ascontiguousarray(p.transpose(2, 1, 0)).reshape(-1)          # [4 x m x N]
    met, cost = np.empty((5, m, n)), np.empty((m, n))
    status, counts = np.empty((m, n), dtype=np.int32), np.empty((2, m, n), dtype=np.int32)
    check(lib.fb_lss_dpid_metrics(world._h, iu, iy, _pd(w), w.size, t_sim, _pd(wt), _pd(flat), None if bnd is None else _pd(bnd), m,
                                  _pd(met), _pd(cost), _pi(counts), _pi(status)))
    return DPIDMetricsResult(metrics=met.transpose(2, 1, 0).copy(), cost=cost.T.copy(), status=status.T.copy(),
                             counts=counts.transpose(2, 1, 0).copy())


def _search_box(settings: Settings):
    lo, hi = np.asarray(settings.lower_bounds, dtype=np.float64), np.asarray(settings.upper_bounds, dtype=np.float64)
    if lo.shape != (4,) or hi.shape != (4,):
        raise ValueError("optimize_dpid: lower_bounds and upper_bounds are PIDData (4 numbers)")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError(f"optimize_dpid: bounds must be finite with lower <= upper, got {lo} and {hi}")
    if not lo[3] >= 0.0:
        raise ValueError(f"optimize_dpid: the lower bound of τ_f = {lo[3]} must not be negative")
    return lo, hi


def optimize_dpid(world, u=0, y=0, data_0=None, settings: Settings | None = None, weights=None, bounds=None, w=None) -> PIDOptResult:
    """optimize_PID under the sampled law for every system of a sampled `world`: one pattern search per system
    (flightbatch.pidopt.pattern_search, which never accepts a worse point), every iteration one fb_lss_dpid_metrics call for the whole
    batch. data_0: a PIDData (or 4 numbers) for the batch, or [N, 4]. bounds: the output bounds of dpid_metrics, a number or [N] a side."""
    settings = settings or Settings()
    lo, hi = _search_box(settings)
    wt = _weights(weights)
    d0 = np.asarray(PIDData() if data_0 is None else data_0, dtype=np.float64)
    if d0.shape not in ((4,), (world.n, 4)):
        raise ValueError(f"optimize_dpid: data_0 must be a PIDData or [N = {world.n}, 4], got {d0.shape}")
    run = lambda pts: dpid_metrics(world, pts, u=u, y=y, settings=settings, weights=wt, bounds=bounds, w=w)
    x, f, evals, iters, done = pattern_search(lambda pts: run(pts).cost, world.n, d0, lo, hi, settings.max_iters)
    last = run(x[:, None, :])
    return PIDOptResult(data=x, cost=last.cost[:, 0], metrics=last.metrics[:, 0], evals=evals, iters=iters,
                        exit_flag=np.where(done, "STEP_TOL_REACHED", "MAXITER_REACHED"), status=last.status[:, 0])
