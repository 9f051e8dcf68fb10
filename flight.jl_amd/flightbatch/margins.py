"""Gain and phase margins of a batch of loops on the device (include/flightbatch.h: fb_lss_margins; kernel: csrc/margins_kernels.hpp;
docs/design/linearize.md, "Margins on the device").

    reference (FA design/robot2d/robot2d_design.ipynb)                 here
    marginplot(P_v[:η, :v_ref])                                        margins(world, u="v_ref", y="η")
    marginplot(series(C_η2v, P_v2η)) with k_p_η2v = 0.6                margins(world, u="v_ref", y="η", gain=0.6)
    nyquistplot(...; Ms_circles = [1])                                 .ms, .wms (the peak of 1 / |1 + L| over the grid)

The loop is L(jω) = gain · (c inv(jωI - A) b + d) of channel (u, y) of each system of a LinearWorld under negative unity feedback. The
crossings are found in the brackets of the frequency grid and refined by bisection; four numbers per system come home, not the grid.
What the margins do not say: whether the closed loop is stable (flightbatch.poles of the closed loop does), and crossings the grid does
not bracket are not found."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .lss import LinearWorld
from .modeling import _pd, _pi
from .pidopt import _channel, default_grid

NOT_FINITE, SINGULAR, TRUNCATED = _K["FB_MARGINS_NOT_FINITE"], _K["FB_MARGINS_SINGULAR"], _K["FB_MARGINS_TRUNCATED"]
KMAX, NX_MAX, NW_MIN, NW_MAX = _K["FB_MARGINS_KMAX"], _K["FB_MARGINS_NX_MAX"], 2, 1024


@dataclass
class MarginsResult:
    gm: np.ndarray        # [N]  gain margin (a factor) closest to 1 in either direction, +Inf without a phase crossing
    wpc: np.ndarray       # [N]  its phase-crossover frequency, rad/s (NaN without one)
    pm: np.ndarray        # [N]  phase margin of smallest magnitude, degrees in (-180, 180], +Inf without a gain crossing
    wgc: np.ndarray       # [N]  its gain-crossover frequency, rad/s (NaN without one)
    ms: np.ndarray        # [N]  1 / min |1 + L| over the grid
    wms: np.ndarray       # [N]  the grid frequency of that peak
    npc: np.ndarray       # [N]  kept phase crossings (at most KMAX)
    ngc: np.ndarray       # [N]  kept gain crossings
    status: np.ndarray    # [N]  0 or NOT_FINITE, SINGULAR (the system's numbers are NaN), TRUNCATED (more than KMAX crossings of a kind)
    l_pc: np.ndarray      # [N]  L at the selected phase crossing (complex)
    l_gc: np.ndarray      # [N]  L at the selected gain crossing
    gm_all: np.ndarray | None = None    # [N, KMAX] with all=True: every kept crossing in ascending frequency, NaN past the count
    wpc_all: np.ndarray | None = None
    pm_all: np.ndarray | None = None
    wgc_all: np.ndarray | None = None

    @property
    def gm_db(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return 20.0 * np.log10(self.gm)

    @property
    def ok(self) -> np.ndarray:
        return (self.status & (NOT_FINITE | SINGULAR)) == 0

    def show(self, i: int = 0) -> str:
        line = (f"system {i}: GM {self.gm[i]:.4g} ({self.gm_db[i]:.2f} dB) at {self.wpc[i]:.4g} rad/s, PM {self.pm[i]:.2f} deg at "
                f"{self.wgc[i]:.4g} rad/s, Ms {self.ms[i]:.3f} at {self.wms[i]:.4g} rad/s; {self.npc[i]} phase and {self.ngc[i]} gain "
                f"crossings, status {self.status[i]}")
        print(line)
        return line


def _margin_grid(w) -> np.ndarray:
    w = default_grid() if w is None else np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 1 or not NW_MIN <= w.size <= NW_MAX:
        raise ValueError(f"margins: the frequency grid must be 1-D with {NW_MIN} to {NW_MAX} entries, got shape {w.shape}")
    if not (np.isfinite(w).all() and (w > 0.0).all() and (np.diff(w) > 0.0).all()):
        raise ValueError("margins: the frequencies must be positive, finite and strictly increasing")
    return w


def _margins_call(fn, world, iu, iy, w, gain, all) -> MarginsResult:
    """what margins and dmargins share once the world, the channel and the grid are checked: the gain for the batch, the output buffers,
    the call of fn (fb_lss_margins or fb_lss_dmargins: one signature) and the result"""
    n = world.n
    if gain is not None:
        gain = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64), (n,)))
    sel, counts, status = np.empty((10, n)), np.empty((2, n), dtype=np.int32), np.empty(n, dtype=np.int32)
    every = np.empty((6, KMAX, n)) if all else None
    check(fn(world._h, iu, iy, _pd(w), w.size, None if gain is None else _pd(gain), _pd(sel), _pi(counts),
             None if every is None else _pd(every), _pi(status)))
    with np.errstate(divide="ignore", invalid="ignore"):
        res = MarginsResult(gm=sel[0].copy(), wpc=sel[1].copy(), pm=sel[2].copy(), wgc=sel[3].copy(), ms=1.0 / sel[8], wms=sel[9].copy(),
                            npc=counts[0].copy(), ngc=counts[1].copy(), status=status, l_pc=sel[4] + 1j * sel[5], l_gc=sel[6] + 1j * sel[7])
        if every is not None:
            res.wpc_all, res.wgc_all = every[0].T.copy(), every[3].T.copy()
            res.gm_all = (-1.0 / every[1]).T.copy()
            res.pm_all = np.degrees(np.arctan2(-every[5], -every[4])).T.copy()
    return res


def margins(world, u=0, y=0, w=None, gain=None, all=False) -> MarginsResult:
    """gain and phase margins of L = gain · P[y, u] of every system of a continuous LinearWorld. u, y: indices or labels; w: the grid in
    rad/s (default pidopt.default_grid()); gain: None (ones), a number for the batch or [N]; all=True also returns every kept crossing."""
    if not isinstance(world, LinearWorld):
        raise FlightBatchError("margins: the world is not a LinearizedSS handle (FB_MODEL_LSS): give it a LinearWorld")
    iu, iy = _channel(world, u, y)
    return _margins_call(lib.fb_lss_margins, world, iu, iy, _margin_grid(w), gain, all)
