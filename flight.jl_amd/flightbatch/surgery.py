"""Design-model surgery for batches of linear models on the device (include/flightbatch.h: fb_lss_transform, fb_lss_steady; kernels:
csrc/surgery_kernels.hpp; docs/design/linearize.md, "Design-model surgery on the device").

    reference                                                                          here
    get_design_model!(ac, trim; model)      FA design/c172/c172x_design.jl:23-82       c172x_design_model(linear_world(world), model)
    T = C[xp_labels, :]; T A inv(T), ...    :49-56                                     transform(world, states, xdot_zero)
    subsystem(lss; x, u, y)                 FP/linearization.jl:113-132                subsystem_world(world, x=, u=, y=)
    delete_vars(lss, s)                     :134-148                                   delete_vars_world(world, names)
    M = inv([A B; C D]); M22 + K M12        design :184-188, :371-381                  steady_state(world, z, K)
    A_aug, B_aug                            :354-355                                   integral_augmentation(world, z)
    LQRDataPoint(K_fbk, K_fwd, K_int)       :149-216, :328-427, :433-536               lqr_tracker(world, z, Q, R, Q_int)

The models stay on the device from linearize to the gains: linearize -> linear_world -> c172x_design_model -> lqr_tracker brings home
K_fbk, K_fwd and K_int only."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .connect import _gain, _static_world, connect
from .lqr import lqr
from .lss import LinearWorld, unpack_matrix
from .modeling import _pd, _pi

SINGULAR, NOT_FINITE, N_MAX = _K["FB_SURGERY_SINGULAR"], _K["FB_SURGERY_NOT_FINITE"], _K["FB_SURGERY_N_MAX"]


@dataclass
class TransformResult:
    world: LinearWorld     # the new models, an ordinary LinearWorld
    status: np.ndarray     # [N]  0, FB_SURGERY_SINGULAR or FB_SURGERY_NOT_FINITE (that system's A, B, C, D, xdot0 are NaN)
    rpiv: np.ndarray       # [N]  smallest pivot magnitude of T over the largest: the warning of a nearly singular T

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0


@dataclass
class SteadyResult:
    X: np.ndarray              # [N, nx, nz]  M12: the states held by a unit of each z
    U: np.ndarray              # [N, nu, nz]  M22: the inputs that hold it
    K_fwd: np.ndarray | None   # [N, nu, nz]  U + K X (None without K)
    status: np.ndarray         # [N]  0, FB_SURGERY_SINGULAR or FB_SURGERY_NOT_FINITE (X, U, K_fwd are NaN there)
    rpiv: np.ndarray           # [N]  smallest pivot magnitude of [A B; C_z D_z] over the largest

    @property
    def ok(self) -> np.ndarray:
        return self.status == 0


def _pick(entries, labels, what, verb):
    """(indices, labels) of a selection given as indices or labels (None: all of them)"""
    if entries is None:
        return None, tuple(labels)
    entries = [entries] if isinstance(entries, str) else list(entries)
    out = []
    for e in entries:
        if isinstance(e, str):
            if e not in labels:
                raise KeyError(f"{verb}: {e!r} is not {what} label of the world")
            out.append(labels.index(e))
        else:
            out.append(int(e))
    return np.array(out, dtype=np.int32), tuple(labels[k] if 0 <= k < len(labels) else None for k in out)


def _lss_world(world, verb):
    if not isinstance(world, LinearWorld):
        raise FlightBatchError(f"{verb}: the world is not a LinearizedSS handle (FB_MODEL_LSS): give it a LinearWorld")


def _transform(verb, world, rows, new_x_labels, zero, x, u, y) -> TransformResult:
    ix, xl = _pick(x, new_x_labels, "a state", verb)
    iu, ul = _pick(u, world.u_labels, "an input", verb)
    iy, yl = _pick(y, world.y_labels, "an output", verb)
    status, rpiv = np.empty(world.n, dtype=np.int32), np.empty(world.n)
    h = C.c_void_p()
    opt = lambda a: (None, 0) if a is None else (_pi(a), len(a))
    check(lib.fb_lss_transform(world._h, None if rows is None else _pi(rows), None if zero is None else _pi(zero), *opt(ix), *opt(iu), *opt(iy),
                               _pi(status), _pd(rpiv), C.byref(h)))
    return TransformResult(world=LinearWorld(_handle=h, _labels=(xl, ul, yl)), status=status, rpiv=rpiv)


def transform(world: LinearWorld, states, xdot_zero=(), x=None, u=None, y=None) -> TransformResult:
    """the change of state variables x' = y[states] (T = C[states, :]: T A inv(T), T B, C inv(T), D; x0' = y0[states], xdot0' = T xdot0
    with the entries named in xdot_zero exactly 0), then subsystem(x=, u=, y=) of the result, on the device. states: nx output labels or
    indices, which become the new state labels; xdot_zero and x: new state labels or indices; u, y: labels or indices of the world.
    D[states, :] is ignored, as the reference ignores it."""
    _lss_world(world, "transform")
    rows, new_x = _pick(states, world.y_labels, "an output", "transform")
    if rows is None or len(rows) != world.nx:
        raise ValueError(f"transform: {0 if rows is None else len(rows)} new states for a world of {world.nx}")
    iz, _ = _pick(list(xdot_zero), new_x, "a new state", "transform")
    if ((iz < 0) | (iz >= world.nx)).any():
        raise ValueError(f"transform: xdot_zero names new states {iz.tolist()}, the world has {world.nx}")
    zero = np.zeros(world.nx, dtype=np.int32)
    zero[iz] = 1
    return _transform("transform", world, rows, new_x, zero, x, u, y)


def subsystem_world(world: LinearWorld, x=None, u=None, y=None) -> LinearWorld:
    """subsystem(lss; x, u, y) of a LinearWorld, device to device: the rows and columns of the named variables in the order given, copies bit for bit"""
    _lss_world(world, "subsystem_world")
    return _transform("subsystem_world", world, None, world.x_labels, None, x, u, y).world


def delete_vars_world(world: LinearWorld, names) -> LinearWorld:
    """delete_vars(lss, names) of a LinearWorld, device to device: every named variable leaves each axis it appears on"""
    _lss_world(world, "delete_vars_world")
    names = [names] if isinstance(names, str) else list(names)
    keep = lambda labels: [k for k, s in enumerate(labels) if s not in names]
    return subsystem_world(world, x=keep(world.x_labels), u=keep(world.u_labels), y=keep(world.y_labels))


def steady_state(world: LinearWorld, z, K=None) -> SteadyResult:
    """[X; U] = the last nz columns of inv([A B; C[z, :] D[z, :]]) and K_fwd = U + K X, on the device. z: nu output labels or indices;
    K: [nu, nx] for the batch or [N, nu, nx] per system (fb_lqr's), None: no K_fwd."""
    _lss_world(world, "steady_state")
    iz, _ = _pick(z, world.y_labels, "an output", "steady_state")
    n, nx, nu = world.n, world.nx, world.nu
    nz = len(iz)
    Kf, kper = (None, 0) if K is None else _gain(K, n, nu, nx, "K", "steady_state")
    X, U, Kfwd = np.empty(nx * nz * n), np.empty(nu * nz * n), (np.empty(nu * nz * n) if K is not None else None)
    status, rpiv = np.empty(n, dtype=np.int32), np.empty(n)
    check(lib.fb_lss_steady(world._h, _pi(iz), nz, None if Kf is None else _pd(Kf), kper, _pd(X), _pd(U), None if Kfwd is None else _pd(Kfwd),
                            _pd(rpiv), _pi(status)))
    return SteadyResult(X=unpack_matrix(X, nx, nz), U=unpack_matrix(U, nu, nz), K_fwd=None if Kfwd is None else unpack_matrix(Kfwd, nu, nz),
                        status=status, rpiv=rpiv)


def integrators_world(n: int, k: int, device: int = 0) -> LinearWorld:
    """n copies of k parallel 1 / s: ξ' = e, y = ξ"""
    eye = np.broadcast_to(np.eye(k), (n, k, k)).copy()
    xi = tuple(f"ξ{j}" for j in range(k))
    return _static_world(n, np.zeros((n, k, k)), eye, eye.copy(), np.zeros((n, k, k)), xi, tuple(f"e{j}" for j in range(k)), xi, device)


def integral_augmentation(world: LinearWorld, z, device: int = 0) -> LinearWorld:
    """the world with an integrator behind each output z (reference: A_aug = [A 0; C_z 0], B_aug = [B; D_z]), by connect: e = y[z] into
    the integrators, w = u. States [x; ξ_z], the world's inputs and outputs (deviation coordinates, as every connected world)."""
    _lss_world(world, "integral_augmentation")
    iz, zl = _pick(z, world.y_labels, "an output", "integral_augmentation")
    k, nu = len(iz), world.nu
    integ = integrators_world(world.n, k, device)
    F = np.vstack([np.zeros((nu, k)), np.eye(k)])
    G = np.vstack([np.eye(nu), np.zeros((k, nu))])
    try:
        res = connect(world, integ, feedback=F, inputs=G, reads=iz, outputs=list(range(world.ny)), input_labels=world.u_labels)
    finally:
        integ.close()
    if not res.ok.all():
        bad = np.flatnonzero(~res.ok)
        res.world.close()
        raise FlightBatchError(f"integral_augmentation: connect flagged systems {bad.tolist()} (status {res.status[bad].tolist()})")
    aug = res.world
    aug.x_labels = tuple(world.x_labels) + tuple(f"ξ_{s}" for s in zl)
    return aug


def lqr_tracker(world: LinearWorld, z, Q, R, Q_int=None, forward: str = "inverse", device: int = 0):
    """(K_fbk [N, nu, nx], K_fwd [N, nu, nz], K_int [N, nu, nz], status [N]) of the tracker u = K_fwd z_ref - K_fbk x - K_int ∫(z - z_ref)
    (the reference's LQRDataPoint recipe): lqr on the world (Q_int None: K_int = 0) or on its integral augmentation (Q: the diagonal on x,
    Q_int: the diagonal on the integrators), then K_fwd = M22 + K_fbk M12 by steady_state (forward="inverse") or K_fwd = I
    (forward="identity", the reference's ar2ar: z are the commands themselves). status: fb_lqr's bits, or FB_SURGERY_* shifted left by 8
    where the steady-state map is flagged."""
    _lss_world(world, "lqr_tracker")
    if forward not in ("inverse", "identity"):
        raise ValueError('lqr_tracker: forward is "inverse" or "identity"')
    iz, _ = _pick(z, world.y_labels, "an output", "lqr_tracker")
    nx, nz = world.nx, len(iz)
    if Q_int is None:
        res = lqr(world, Q, R)
        K_fbk, K_int = res.K, np.zeros((world.n, world.nu, nz))
    else:
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim != 1:
            raise ValueError("lqr_tracker: with Q_int, Q is the diagonal on the states")
        aug = integral_augmentation(world, iz, device)
        try:
            res = lqr(aug, np.concatenate([Q, np.asarray(Q_int, dtype=np.float64)]), R)
        finally:
            aug.close()
        K_fbk, K_int = np.ascontiguousarray(res.K[:, :, :nx]), np.ascontiguousarray(res.K[:, :, nx:])
    if forward == "identity":
        if nz != world.nu:
            raise ValueError(f"lqr_tracker: forward=\"identity\" takes as many z as inputs ({world.nu}), got {nz}")
        return K_fbk, np.broadcast_to(np.eye(nz), (world.n, nz, nz)).copy(), K_int, res.status.copy()
    st = steady_state(world, iz, np.where(np.isfinite(K_fbk), K_fbk, 0.0))
    K_fwd = np.where((res.status == 0)[:, None, None], st.K_fwd, np.nan)
    return K_fbk, K_fwd, K_int, res.status | (st.status << 8)


# get_design_model! (FA design/c172/c172x_design.jl:36-75)
_C172X_SWAP = {"v_x": "EAS", "v_y": "α", "v_z": "β", "ω_eng": "n_eng"}
_C172X_LON = ("q", "θ", "EAS", "α", "h", "α_filt", "n_eng", "thr_p", "ele_p")
_C172X_LAT = ("p", "r", "ψ", "φ", "EAS", "β", "β_filt", "ail_p", "rud_p")
_C172X_MODELS = {
    "full": (None, None, None),
    "lon": (_C172X_LON, ("throttle_cmd", "elevator_cmd"), _C172X_LON + ("f_x", "f_z", "TAS", "γ", "climb_rate", "throttle_cmd", "elevator_cmd")),
    "lat": (_C172X_LAT, ("aileron_cmd", "rudder_cmd"), _C172X_LAT + ("f_y", "χ", "aileron_cmd", "rudder_cmd")),
}


def c172x_design_model(world: LinearWorld, model: str = "full") -> TransformResult:
    """get_design_model!(aircraft, trim; model) for the LinearWorld of a Cessna172Xv2 linearisation (linear_world(world) after
    linearize): (v_x, v_y, v_z, ω_eng) give way to (EAS, α, β, n_eng) as states, whose xdot0 is exactly 0 (guaranteed by the trim
    constraints); model "lon" / "lat": the reference's longitudinal / lateral subsystem."""
    if model not in _C172X_MODELS:
        raise ValueError('c172x_design_model: valid models are "full", "lon", "lat"')
    _lss_world(world, "c172x_design_model")
    states = [_C172X_SWAP.get(s, s) for s in world.x_labels]
    x, u, y = _C172X_MODELS[model]
    return transform(world, states, xdot_zero=tuple(_C172X_SWAP.values()), x=x, u=u, y=y)
