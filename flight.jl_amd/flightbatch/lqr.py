"""lqr(P, Q, R) for a batch of linear models on the device (include/flightbatch.h: fb_lqr; kernels: csrc/lqr_kernels.hpp;
docs/design/linearize.md, "LQR design on the device").

    reference                                                               here
    lqr(P, Q, R)                FA design/c172/c172x_design.jl:181, 369, ...   lqr(world, Q, R)            world = LinearWorld(lss) / linear_world(...)
    the loop closed on u = -K x                                              closed_loop(lss, K)         -> LinearizedSS, steps as a LinearWorld

The design scripts' model surgery (the similarity transform to (EAS, α, β, n_eng), the integral augmentation, K_fwd) is on the device in
flightbatch.surgery (transform, integral_augmentation, steady_state, lqr_tracker); it can still be done in host-side numpy on the
LinearizedSS before it goes to the device. A model that exists only to be designed on still needs outputs (fb_lss_create wants ny >= 1):
give it C = I, D = 0, as design_model does."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .linearization import LinearizedSS
from .lss import LinearWorld, unpack_matrix
from .modeling import _pd, _pi


@dataclass
class LqrResult:
    K: np.ndarray        # [N, nu, nx]   u = -K x
    X: np.ndarray        # [N, nx, nx]   the stabilising solution of the Riccati equation
    resid: np.ndarray    # [N]           max|A'X + XA - XGX + Q| / max(max|Q|, max|X|)
    iters: np.ndarray    # [N]           Newton iterations of the matrix sign function
    status: np.ndarray   # [N]           0, or FB_LQR_NOT_CONVERGED | FB_LQR_SINGULAR (K, X, resid are NaN there)

    @property
    def success(self) -> np.ndarray:
        return self.status == 0


def _weight(M, n: int, name: str) -> np.ndarray:
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 1:
        M = np.diag(M)
    if M.shape != (n, n):
        raise ValueError(f"lqr: {name} must be {n} x {n} (or its diagonal), got {M.shape}")
    return np.asfortranarray(M)


def lqr(world: LinearWorld, Q, R) -> LqrResult:
    """K = lqr(A, B, Q, R) of every system of `world`, on its device. Q [nx, nx] and R [nu, nu] are the batch's (1-D: a diagonal)."""
    n, nx, nu = world.n, world.nx, world.nu
    Q, R = _weight(Q, nx, "Q"), _weight(R, nu, "R")
    Kf, Xf = np.empty(nu * nx * n), np.empty(nx * nx * n)
    resid, iters, status = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    check(lib.fb_lqr(world._h, _pd(Q.reshape(-1, order="F")), _pd(R.reshape(-1, order="F")), _pd(Kf), _pd(Xf), _pd(resid), _pi(iters), _pi(status)))
    return LqrResult(K=unpack_matrix(Kf, nu, nx), X=unpack_matrix(Xf, nx, nx), resid=resid, iters=iters, status=status)


def closed_loop(lss: LinearizedSS, K) -> LinearizedSS:
    """the model with u = u0 - K (x - x0) + v closed around it: A - B K, C - D K, xdot0 = 0 (the design point is its equilibrium); v takes u's
    place as the input. Host-side numpy; LinearWorld(closed_loop(lss, K)) steps the designed loop."""
    K = np.asarray(K, dtype=np.float64)
    A, B, C, D = (np.asarray(m, dtype=np.float64) for m in (lss.A, lss.B, lss.C, lss.D))
    if K.ndim == 2:
        K = np.broadcast_to(K, (A.shape[0],) + K.shape)
    return replace(lss, A=A - B @ K, C=C - D @ K, xdot0=np.zeros_like(np.asarray(lss.xdot0, dtype=np.float64)))


def design_model(A, B, x0=None, x_labels=None, u_labels=None) -> LinearizedSS:
    """a LinearizedSS to design on from A [N, nx, nx] and B [N, nx, nu] alone: C = I, D = 0, equilibrium at x0 (default 0), u0 = 0"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, nx, nu = B.shape
    x0 = np.zeros((n, nx)) if x0 is None else np.asarray(x0, dtype=np.float64)
    xl = tuple(x_labels) if x_labels is not None else tuple(f"x{k}" for k in range(nx))
    ul = tuple(u_labels) if u_labels is not None else tuple(f"u{k}" for k in range(nu))
    return LinearizedSS(xdot0=np.zeros((n, nx)), x0=x0, u0=np.zeros((n, nu)), y0=x0.copy(), A=A, B=B,
                        C=np.broadcast_to(np.eye(nx), (n, nx, nx)).copy(), D=np.zeros((n, nx, nu)), x_labels=xl, u_labels=ul, y_labels=xl)


NOT_CONVERGED, SINGULAR, NX_MAX = _K["FB_LQR_NOT_CONVERGED"], _K["FB_LQR_SINGULAR"], _K["FB_LQR_NX_MAX"]


# ---- the discrete side: lqr(Discrete, Phi, Gamma, Q, R) on a sampled world (include/flightbatch.h: fb_lss_dlqr; kernel: csrc/dlqr_kernels.hpp;
# docs/design/linearize.md, "Discrete LQR on the device") ---------------------------------------------------------------------------------
@dataclass
class DlqrResult:
    K: np.ndarray        # [N, nu, nx]   u = u0 - K (x - x0), held between samples
    X: np.ndarray        # [N, nx, nx]   the stabilising solution of the discrete Riccati equation
    resid: np.ndarray    # [N]           max|Phi'X Phi - X - Phi'X Gamma K + Q| / max(max|Q|, max|X|)
    iters: np.ndarray    # [N]           doublings taken
    status: np.ndarray   # [N]           0, or FB_DLQR_NOT_CONVERGED | FB_DLQR_SINGULAR (K, X, resid are NaN there)
    world: LinearWorld | None = None     # closed=True: the designed loop, a sampled LinearWorld (Phi - Gamma K, C - D K), labels carried over

    @property
    def success(self) -> np.ndarray:
        return self.status == 0


def dlqr(world: LinearWorld, Q, R, closed: bool = False) -> DlqrResult:
    """K = lqr(Discrete, Phi, Gamma, Q, R) of every system of a sampled `world` (c2d(w, Ts).world), on its device. Q [nx, nx] and R [nu, nu]
    are the batch's (1-D: a diagonal). With closed=True the result's `world` is the designed loop as a sampled LinearWorld of its own."""
    if not isinstance(world, LinearWorld):
        raise FlightBatchError("dlqr: the world is not a LinearizedSS handle (FB_MODEL_LSS): give it a sampled LinearWorld (c2d(w, Ts).world)")
    n, nx, nu = world.n, world.nx, world.nu
    Q, R = _weight(Q, nx, "Q"), _weight(R, nu, "R")
    Kf, Xf = np.empty(nu * nx * n), np.empty(nx * nx * n)
    resid, iters, status = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    h = C.c_void_p()
    check(lib.fb_lss_dlqr(world._h, _pd(Q.reshape(-1, order="F")), _pd(R.reshape(-1, order="F")), _pd(Kf), _pd(Xf), _pd(resid), _pi(iters), _pi(status),
                          C.byref(h) if closed else None))
    w = LinearWorld(_handle=h, _labels=(tuple(world.x_labels), tuple(world.u_labels), tuple(world.y_labels))) if closed else None
    return DlqrResult(K=unpack_matrix(Kf, nu, nx), X=unpack_matrix(Xf, nx, nx), resid=resid, iters=iters, status=status, world=w)


DLQR_NOT_CONVERGED, DLQR_SINGULAR, DLQR_NX_MAX, DLQR_MAX_ITERS = (_K["FB_DLQR_NOT_CONVERGED"], _K["FB_DLQR_SINGULAR"], _K["FB_DLQR_NX_MAX"],
                                                                  _K["FB_DLQR_MAX_ITERS"])
