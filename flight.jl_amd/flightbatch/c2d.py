"""Sampled models on the device: zero-order-hold discretisation of a batch of linear models (include/flightbatch.h: fb_lss_c2d,
fb_lss_sample_time; kernels: csrc/c2d_kernels.hpp, fbz::k_lss_map, fbz::k_timeresp_map; docs/design/linearize.md, "Sampled models on the
device").

    reference                                                                     here
    c2d(sys, Ts) (what step and lsim do before they simulate)                      c2d(world, Ts).world
    step(T, t_sim)           FA design/pidopt.jl, robot2d_design.ipynb            timeresp.step(world, channels, t_sim, dt, method="zoh")
    lsim(e2q, (x, t) -> [0.1] * (t >= 1), 0:0.01:10)   demos/c172_demos.jl        timeresp.lsim(world, 0.1 * (t >= 1), t)

The sampled world is an ordinary LinearWorld whose model() returns (Phi, Gamma): step() applies x+ = x0 + Phi (x - x0) + Gamma (u - u0) +
delta and advances the clock by Ts, f_ode() refreshes y, timeresp.step / stepinfo sample the map. The continuous-time design verbs (lqr,
poles, connect, transform, ...) refuse it by name."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .lss import LinearWorld
from .modeling import _pi

NOT_FINITE, RANGE, SQUARINGS_MAX = _K["FB_C2D_NOT_FINITE"], _K["FB_C2D_RANGE"], _K["FB_C2D_SQUARINGS_MAX"]


@dataclass
class C2dResult:
    world: LinearWorld       # the sampled models: world.Ts == Ts, world.squarings is `squarings`
    status: np.ndarray       # [N]  0, FB_C2D_NOT_FINITE or FB_C2D_RANGE (that system's Phi, Gamma and delta are NaN)
    squarings: np.ndarray    # [N]  s of the scaling and squaring (0 where there is a status)

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0

    @property
    def Ts(self) -> float:
        return self.world.Ts


def c2d(world: LinearWorld, Ts: float) -> C2dResult:
    """the zero-order-hold sampled model of every system of a continuous LinearWorld at sample time Ts, device to device; labels are
    carried over"""
    if not isinstance(world, LinearWorld):
        raise FlightBatchError("c2d: the world is not a LinearizedSS handle (FB_MODEL_LSS): give it a LinearWorld")
    status, squarings = np.empty(world.n, dtype=np.int32), np.empty(world.n, dtype=np.int32)
    h = C.c_void_p()
    check(lib.fb_lss_c2d(world._h, float(Ts), _pi(squarings), _pi(status), C.byref(h)))
    w = LinearWorld(_handle=h, _labels=(tuple(world.x_labels), tuple(world.u_labels), tuple(world.y_labels)))
    w.squarings = squarings
    return C2dResult(world=w, status=status, squarings=squarings)
