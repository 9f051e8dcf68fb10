"""Sampled loops on the device: frequency response, margins and poles of a batch of sampled models (include/flightbatch.h:
fb_lss_set_sampled, fb_lss_dfreqresp, fb_lss_dmargins, fb_lss_dpoles; kernels: csrc/dfreq_kernels.hpp, and fbe::k_poles for the poles;
docs/design/linearize.md, "Sampled loops on the device").

    reference (ControlSystems on a discrete system)                    here
    freqresp(sysd, w)                                                  dfreqresp(world, u, y, w)
    margin(sysd) / marginplot(sysd)                                    dmargins(world, u, y, gain=...)
    poles(sysd), isstable(sysd)                                        dpoles(world).poles, .stable
    damp(sysd), dampreport(sysd)                                       dpoles(world).wn, .zeta;  print(ddampreport(dpoles(world), i))

The world is a sampled LinearWorld: c2d(world, Ts).world, dlqr(..., closed=True).closed, or LinearWorld(lss, Ts=...) for a model that is
given as (Phi, Gamma) — a loop with a sample of delay has an eigenvalue at 0 and is no zero-order hold of anything. The loop is
L(z) = gain · (c inv(zI - Phi) gamma + d) on z = e^(jωTs), 0 < ω <= π/Ts, under negative unity feedback; frequencies are rad/s in and out.
A phase crossing at the Nyquist frequency itself is not bracketed (L is real there)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import FlightBatchError, check, lib
from .lss import LinearWorld
from .margins import NW_MAX, MarginsResult, _margins_call
from .modeling import _pd, _pi
from .pidopt import _channel
from .poles import _g3

NW_DEFAULT = 321


def default_dgrid(Ts: float, nw: int = NW_DEFAULT) -> np.ndarray:
    """nw frequencies, logarithmic from 1e-4 π/Ts to the Nyquist frequency π/Ts; the last one is lowered, an ulp at a time, until its
    angle ω Ts is at most π in floating point (the library refuses a grid above the Nyquist frequency)"""
    w = np.logspace(-4.0, 0.0, nw) * (np.pi / Ts)
    w[-1] = np.pi / Ts
    while w[-1] * Ts > np.pi:
        w[-1] = np.nextafter(w[-1], 0.0)
    return w


def _sampled(world, verb) -> float:
    if not isinstance(world, LinearWorld):
        raise FlightBatchError(f"{verb}: the world is not a LinearizedSS handle (FB_MODEL_LSS): give it a sampled LinearWorld")
    return world.Ts


def _dgrid(world, w, verb, nw_min) -> np.ndarray:
    if w is None:
        Ts = world.Ts
        if not Ts > 0.0:      # (the library's refusal, before a grid is made of Ts = 0)
            raise FlightBatchError(f"{verb}: a discrete-time verb on a continuous model: sample it first (c2d, or LinearWorld(lss, Ts=...))")
        return default_dgrid(Ts)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 1 or not nw_min <= w.size <= NW_MAX:
        raise ValueError(f"{verb}: the frequency grid must be 1-D with {nw_min} to {NW_MAX} entries, got shape {w.shape}")
    return w


def dfreqresp(world, u, y, w) -> np.ndarray:
    """P(e^(jωTs)) of channel (u, y) of every system of a sampled LinearWorld on the grid w (rad/s, at most π/Ts): complex [nw, N]"""
    _sampled(world, "dfreqresp")
    iu, iy = _channel(world, u, y)
    w = _dgrid(world, w, "dfreqresp", 1)
    re, im = np.empty((w.size, world.n)), np.empty((w.size, world.n))
    check(lib.fb_lss_dfreqresp(world._h, iu, iy, _pd(w), w.size, _pd(re), _pd(im)))
    return re + 1j * im


def dmargins(world, u=0, y=0, w=None, gain=None, all=False) -> MarginsResult:
    """gain and phase margins of L = gain · P[y, u] of every system of a sampled LinearWorld. u, y: indices or labels; w: the grid in
    rad/s (default default_dgrid(world.Ts)); gain: None (ones), a number for the batch or [N]; all=True also returns every kept crossing."""
    _sampled(world, "dmargins")
    iu, iy = _channel(world, u, y)
    return _margins_call(lib.fb_lss_dmargins, world, iu, iy, _dgrid(world, w, "dmargins", 2), gain, all)


@dataclass
class DPolesResult:
    poles: np.ndarray    # [N, nx] complex128: the eigenvalues z of Phi, ascending by |z|, then Re, then Im; NaN where status != 0
    iters: np.ndarray    # [N]     QR sweeps taken
    status: np.ndarray   # [N]     0, or FB_POLES_NOT_CONVERGED | FB_POLES_NOT_FINITE
    Ts: float

    @property
    def s(self) -> np.ndarray:
        """the s-plane image log(z) / Ts of each pole (principal branch); -Inf + 0j for a pole at 0"""
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.log(self.poles)
        s = np.empty_like(lg)
        s.real, s.imag = lg.real / self.Ts, lg.imag / self.Ts      # (component by component: a complex division of -Inf + 0j gives NaN)
        return s

    @property
    def wn(self) -> np.ndarray:
        """natural frequency |s|, rad/s (+Inf for a pole at 0)"""
        return np.abs(self.s)

    @property
    def zeta(self) -> np.ndarray:
        """damping ratio -cos(arg s) (1 for a pole at 0)"""
        s = self.s
        return -np.cos(np.arctan2(s.imag, s.real))

    @property
    def tau(self) -> np.ndarray:
        """time constant -1 / Re s, s (0 for a pole at 0)"""
        with np.errstate(divide="ignore"):
            return -1.0 / self.s.real

    @property
    def stable(self) -> np.ndarray:
        """[N] status 0 and every pole inside the unit circle"""
        with np.errstate(invalid="ignore"):
            return (self.status == 0) & (np.abs(self.poles).max(axis=1) < 1.0)


def dpoles(world: LinearWorld) -> DPolesResult:
    """the nx eigenvalues of Phi of every system of a sampled `world`, on its device, with damp's z-plane reading"""
    Ts = _sampled(world, "dpoles")
    n, nx = world.n, world.nx
    re, im = np.empty(nx * n), np.empty(nx * n)
    iters, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    check(lib.fb_lss_dpoles(world._h, _pd(re), _pd(im), _pi(iters), _pi(status)))
    return DPolesResult(poles=(re + 1j * im).reshape(nx, n).T.copy(), iters=iters, status=status, Ts=Ts)


def ddampreport(result: DPolesResult, i: int = 0) -> str:
    """the reference's table for system i of a discrete system, sorted by natural frequency: pole (in z), damping ratio, frequency in
    rad/s and Hz, time constant"""
    out = ["|        Pole        |   Damping     |   Frequency   |   Frequency   | Time Constant |",
           "|                    |    Ratio      |   (rad/sec)   |     (Hz)      |     (sec)     |",
           "+--------------------+---------------+---------------+---------------+---------------+"]
    wn, zeta, tau = result.wn[i], result.zeta[i], result.tau[i]
    for k in np.argsort(wn, kind="stable"):
        lam = result.poles[i][k]
        if np.isnan(lam.real):
            pole = "NaN"
        else:
            pole = ("-" if np.signbit(lam.real) else "+") + _g3(abs(lam.real))
            if lam.imag != 0.0:
                pole = "%-7s %s %-6sim" % (pole, "-" if lam.imag < 0 else "+", _g3(abs(lam.imag)))
        out.append("| %-19s|  %-13s|  %-13s|  %-13s|  %-13s|" % (pole, _g3(zeta[k]), _g3(wn[k]), _g3(wn[k] / (2 * np.pi)), _g3(tau[k])))
    return "\n".join(out)
