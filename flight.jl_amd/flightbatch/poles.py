"""The poles of a batch of linear models on the device, and dampreport's table of them (include/flightbatch.h: fb_lss_poles; kernels:
csrc/poles_kernels.hpp; docs/design/linearize.md, "Poles on the device").

    reference                                                               here
    dampreport(P)        FA design/robot2d/robot2d_design.ipynb             print(dampreport(poles(world), i))     world = LinearWorld(lss) / linear_world(...)
    poles(P), isstable(P)                                                   poles(world).poles, .stable

The natural frequency, damping ratio and time constant are host-side arithmetic on the poles the device returns."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, check, lib
from .lss import LinearWorld
from .modeling import _pd, _pi


@dataclass
class PolesResult:
    poles: np.ndarray    # [N, nx] complex128, ascending by |pole|, then Re, then Im; NaN where status != 0
    iters: np.ndarray    # [N]     QR sweeps taken
    status: np.ndarray   # [N]     0, or FB_POLES_NOT_CONVERGED | FB_POLES_NOT_FINITE

    @property
    def wn(self) -> np.ndarray:
        """natural frequency |pole|, rad/s"""
        return np.abs(self.poles)

    @property
    def zeta(self) -> np.ndarray:
        """damping ratio -cos(arg pole): 1 for a stable real pole, -1 for an unstable one and for a pole at +0"""
        return -np.cos(np.angle(self.poles))

    @property
    def tau(self) -> np.ndarray:
        """time constant -1 / Re pole, s (-Inf for a pole at +0)"""
        with np.errstate(divide="ignore"):
            return -1.0 / self.poles.real

    @property
    def stable(self) -> np.ndarray:
        """[N] status 0 and every pole in the open left half plane"""
        with np.errstate(invalid="ignore"):
            return (self.status == 0) & (self.poles.real.max(axis=1) < 0.0)


def poles(world: LinearWorld) -> PolesResult:
    """the nx eigenvalues of A of every system of `world`, on its device"""
    n, nx = world.n, world.nx
    re, im = np.empty(nx * n), np.empty(nx * n)
    iters, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    check(lib.fb_lss_poles(world._h, _pd(re), _pd(im), _pi(iters), _pi(status)))
    lam = (re + 1j * im).reshape(nx, n).T.copy()
    return PolesResult(poles=lam, iters=iters, status=status)


def _g3(v: float) -> str:
    """three significant digits as the reference prints them (%.3g; its infinities are Inf)"""
    if np.isinf(v):
        return "Inf" if v > 0 else "-Inf"
    if np.isnan(v):
        return "NaN"
    s = "%.3g" % v
    return "0" if s == "-0" else s


def dampreport(result: PolesResult, i: int = 0) -> str:
    """the reference's table for system i: pole, damping ratio, frequency in rad/s and Hz, time constant"""
    out = ["|        Pole        |   Damping     |   Frequency   |   Frequency   | Time Constant |",
           "|                    |    Ratio      |   (rad/sec)   |     (Hz)      |     (sec)     |",
           "+--------------------+---------------+---------------+---------------+---------------+"]
    for lam, wn, zeta, tau in zip(result.poles[i], result.wn[i], result.zeta[i], result.tau[i]):
        if np.isnan(lam.real):
            pole = "NaN"
        else:
            pole = ("-" if np.signbit(lam.real) else "+") + _g3(abs(lam.real))
            if lam.imag != 0.0:      # (this project's layout: the tables the reference stores hold real poles only)
                pole = "%-7s %s %-6sim" % (pole, "-" if lam.imag < 0 else "+", _g3(abs(lam.imag)))
        out.append("| %-19s|  %-13s|  %-13s|  %-13s|  %-13s|" % (pole, _g3(zeta), _g3(wn), _g3(wn / (2 * np.pi)), _g3(tau)))
    return "\n".join(out)


NOT_CONVERGED, NOT_FINITE, NX_MAX = _K["FB_POLES_NOT_CONVERGED"], _K["FB_POLES_NOT_FINITE"], _K["FB_POLES_NX_MAX"]
