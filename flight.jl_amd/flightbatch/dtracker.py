"""Discrete LQR trackers on the device: the sampled tracker law the stepper flies, on a batch of sampled models, and the sampled design chain
(include/flightbatch.h: fb_lss_dtracker_metrics, fb_lss_dsteady; kernels: csrc/dtracker_kernels.hpp, csrc/surgery_kernels.hpp;
docs/design/linearize.md, "Discrete LQR trackers on the device").

    reference                                                          here
    f_periodic! of LQR                    FP/control.jl:708-743        the law of dtracker_metrics, per (system, candidate) pair
    M = inv([A B; C D]); M22 + K M12      design :184-188, :371-381    dsteady_state(world, z, K, K_xi): the equilibrium of the map
    A_aug, B_aug                          :354-355                     dintegral_augmentation(world, z): states [x_k; ξ_k-1]
    LQRDataPoint(K_fbk, K_fwd, K_int)     :149-216, :328-427           dlqr_tracker(world, z, Q, R, Q_int)
    connect([P, C], ...) of the loop      :199-216                     dtracker_world(world, z, K_fbk, K_fwd, K_int)

The world is a sampled LinearWorld (c2d(world, Ts).world, or LinearWorld(lss, Ts=...)), in deviation coordinates as every connected world.
Per tick of Ts the law reads z_k = C_z x_k + D_z u_k-1 (it samples its command variables before it writes its output), integrates
v_k = K_int (z_ref - z_k) with a rectangular integrator that includes the current sample, clamps u_k = ι_k + K_fwd z_ref - K_fbk x_k per
input and halts an input's integrator while that output is clamped and v pushes further into the bound."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import K as _K, FlightBatchError, check, lib
from .connect import _gain
from .dconnect import _sampled_world, dconnect
from .dfreq import _sampled
from .lqr import dlqr
from .lss import LinearWorld, unpack_matrix
from .modeling import _pd, _pi
from .pidopt import M_MAX
from .surgery import SteadyResult, _pick
from .timeresp import samples

DIVERGED, NOT_FINITE, ROWS_MAX, DIRECT = (_K[k] for k in ("FB_DTRACK_DIVERGED", "FB_DTRACK_NOT_FINITE", "FB_DTRACK_ROWS_MAX", "FB_DSTEADY_DIRECT"))


@dataclass
class DSteadyResult(SteadyResult):
    K_fbk: np.ndarray | None = None   # [N, nu, nx]  K - Ts K_xi C_z (K without K_xi; None without K)


@dataclass
class DTrackerResult:
    t: np.ndarray        # [ns]            sample times: s stride Ts, the last one N_t Ts
    z: np.ndarray        # [N, m, nz, ns]  the command variables
    u: np.ndarray        # [N, m, nu, ns]  the outputs of the law
    ie: np.ndarray       # [N, m, nz]      the trapezoid mean of |z_ref - z|
    ef: np.ndarray       # [N, m, nz]      |z_ref - z| at the last tick
    zp: np.ndarray       # [N, m, nz]      max |z|
    iu: np.ndarray       # [N, m, nu]      the trapezoid mean of |u|
    up: np.ndarray       # [N, m, nu]      max |u|
    clamped: np.ndarray  # [N, m, nu]      ticks with the output clamped (of k = 0 .. N_t)
    halted: np.ndarray   # [N, m, nu]      ticks with the integrator halted
    status: np.ndarray   # [N, m]          0, DIVERGED or NOT_FINITE


def dsteady_state(world: LinearWorld, z, K=None, K_xi=None) -> DSteadyResult:
    """[X; U] = the last nz columns of inv([Phi - I, Gamma; C[z, :], D[z, :]]), K_fbk = K - Ts K_xi C_z (K_xi None: K) and
    K_fwd = U + K_fbk X of a sampled world, on the device. z: nu output labels or indices; K [nu, nx] and K_xi [nu, nz]: for the batch, or
    [N, ...] per system (both alike). A system with K_xi and D_z != 0 is flagged DIRECT: K_fbk and K_fwd NaN, X and U delivered."""
    _sampled(world, "dsteady_state")
    iz, _ = _pick(z, world.y_labels, "an output", "dsteady_state")
    n, nx, nu = world.n, world.nx, world.nu
    nz = len(iz)
    if K_xi is not None and K is None:
        raise ValueError("dsteady_state: K_xi needs K")
    Kf, kper = (None, 0) if K is None else _gain(K, n, nu, nx, "K", "dsteady_state")
    Xi = None
    if K_xi is not None:
        Xi, xper = _gain(K_xi, n, nu, nz, "K_xi", "dsteady_state")
        if xper != kper:
            raise ValueError("dsteady_state: K and K_xi are both for the batch or both per system")
    opt = lambda a: None if a is None else _pd(a)
    X, U = np.empty(nx * nz * n), np.empty(nu * nz * n)
    Kfbk, Kfwd = (np.empty(nu * nx * n), np.empty(nu * nz * n)) if K is not None else (None, None)
    status, rpiv = np.empty(n, dtype=np.int32), np.empty(n)
    check(lib.fb_lss_dsteady(world._h, _pi(iz), nz, opt(Kf), opt(Xi), kper, _pd(X), _pd(U), opt(Kfbk), opt(Kfwd), _pd(rpiv), _pi(status)))
    return DSteadyResult(X=unpack_matrix(X, nx, nz), U=unpack_matrix(U, nu, nz), K_fwd=None if Kfwd is None else unpack_matrix(Kfwd, nu, nz),
                         status=status, rpiv=rpiv, K_fbk=None if Kfbk is None else unpack_matrix(Kfbk, nu, nx))


def _pair_gain(M, n, m, rows, cols, name):
    """[N, m, rows, cols] from [rows, cols] (the batch's), [N, rows, cols] or [N, m, rows, cols]"""
    M = np.asarray(M, dtype=np.float64)
    if M.shape == (rows, cols):
        M = M[None, None]
    elif M.shape == (n, rows, cols):
        M = M[:, None]
    if M.ndim != 4 or M.shape[0] not in (1, n) or M.shape[1] not in (1, m) or M.shape[2:] != (rows, cols):
        raise ValueError(f"dtracker_metrics: {name} must be [{rows}, {cols}], [N = {n}, {rows}, {cols}] or [N, m = {m}, {rows}, {cols}], got {M.shape}")
    return np.broadcast_to(M, (n, m, rows, cols))


def _pack_pairs(M) -> np.ndarray:
    """[N, m, rows, cols] -> flat, element (r, c) of pair (i, j) at [((r + rows c) m + j) N + i]"""
    return np.ascontiguousarray(M.transpose(3, 2, 1, 0)).reshape(-1)


def _u_bounds(bounds, n, m, nu, u_trim):
    """None, or (lo, hi) with each side a number, [nu], [N, nu] or [N, m, nu] (absolute when u_trim [nu] or [N, nu] is given): flat [2 x nu x m x N]"""
    if bounds is None:
        return None
    if len(bounds) != 2:
        raise ValueError("dtracker_metrics: bounds must be None or a pair (lo, hi)")
    trim = 0.0 if u_trim is None else np.asarray(u_trim, dtype=np.float64)
    trim = trim[:, None, :] if np.ndim(trim) == 2 else trim

    def side(v):
        v = np.asarray(v, dtype=np.float64)
        v = v[:, None, :] if v.ndim == 2 else v
        return np.broadcast_to(v - trim, (n, m, nu))
    lo, hi = side(bounds[0]), side(bounds[1])
    if np.isnan(lo).any() or np.isnan(hi).any() or not (lo < hi).all():
        raise ValueError("dtracker_metrics: the output bounds must satisfy lo < hi (either may be infinite)")
    return np.ascontiguousarray(np.stack([lo.transpose(2, 1, 0), hi.transpose(2, 1, 0)])).reshape(-1)


def dtracker_metrics(world: LinearWorld, z, K_fbk, K_fwd, K_int, zref, t_sim: float, bounds=None, stride: int | None = None,
                     u_trim=None) -> DTrackerResult:
    """the step response to z_ref of every (system, candidate) pair of a sampled LinearWorld under the sampled tracker law, its metrics and
    its clamp and halt counts, in one call. z: nz output labels or indices; the gains: [nu, .] for the batch, [N, nu, .] or [N, m, nu, .];
    zref: a number or [nz], the batch's; bounds: None or (lo, hi) on the deviation of u (with u_trim: on u itself), each side a number,
    [nu], [N, nu] or [N, m, nu]; stride: every stride-th sample and the last one come home (None: only the first and the last)."""
    _sampled(world, "dtracker_metrics")
    iz, _ = _pick(z, world.y_labels, "an output", "dtracker_metrics")
    n, nx, nu, nz = world.n, world.nx, world.nu, len(iz)
    m = max([1] + [np.shape(g)[1] for g in (K_fbk, K_fwd, K_int) if np.ndim(g) == 4])
    if not 1 <= m <= M_MAX:
        raise ValueError(f"dtracker_metrics: m = {m}, a call takes 1 to {M_MAX} candidates per system")
    fbk, fwd, kin = (_pack_pairs(_pair_gain(g, n, m, nu, c, name)) for g, c, name in ((K_fbk, nx, "K_fbk"), (K_fwd, nz, "K_fwd"), (K_int, nz, "K_int")))
    bnd = _u_bounds(bounds, n, m, nu, u_trim)
    zr = np.ascontiguousarray(np.broadcast_to(np.asarray(zref, dtype=np.float64), (nz,)))
    Ts, t_sim = float(world.Ts), float(t_sim)
    N = int(round(t_sim / Ts)) if Ts > 0.0 and np.isfinite(t_sim) else 0
    if not 1 <= N <= 200000:
        raise ValueError(f"dtracker_metrics: t_sim = {t_sim} at Ts = {Ts} gives {N} ticks, a call takes 1 to 200000")
    stride = N if stride is None else int(stride)
    ns = samples(N, stride)
    zmet, umet, counts = np.empty((3, nz, m, n)), np.empty((2, nu, m, n)), np.empty((2, nu, m, n), dtype=np.int32)
    zs, us, status = np.empty((ns, nz, m, n)), np.empty((ns, nu, m, n)), np.empty((m, n), dtype=np.int32)
    check(lib.fb_lss_dtracker_metrics(world._h, _pi(iz), nz, _pd(fbk), _pd(fwd), _pd(kin), None if bnd is None else _pd(bnd), m, _pd(zr), t_sim,
                                      stride, _pd(zmet), _pd(umet), _pi(counts), _pd(zs), _pd(us), _pi(status)))
    t = np.arange(ns, dtype=np.float64) * (stride * Ts)
    t[-1] = N * Ts
    home = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))          # [rows, m, N] -> [N, m, rows]
    return DTrackerResult(t=t, z=np.ascontiguousarray(zs.transpose(3, 2, 1, 0)), u=np.ascontiguousarray(us.transpose(3, 2, 1, 0)),
                          ie=home(zmet[0]), ef=home(zmet[1]), zp=home(zmet[2]), iu=home(umet[0]), up=home(umet[1]),
                          clamped=home(counts[0]), halted=home(counts[1]), status=status.T.copy())


def dintegrators_world(n: int, k: int, Ts: float, device: int = 0) -> LinearWorld:
    """n copies of k parallel rectangular integrators that include the current sample: ξ+ = ξ + Ts e, y = ξ + Ts e"""
    eye = np.broadcast_to(np.eye(k), (n, k, k)).copy()
    xi = tuple(f"ξ{j}" for j in range(k))
    return _sampled_world(n, eye, float(Ts) * eye, eye.copy(), float(Ts) * eye, xi, tuple(f"e{j}" for j in range(k)), xi, float(Ts), device)


def dintegral_augmentation(world: LinearWorld, z, device: int = 0) -> LinearWorld:
    """the sampled world with a rectangular integrator behind each output z, by dconnect: e = y[z] into the integrators, w = u. States
    [x_k; ξ_k-1] with ξ_k = ξ_k-1 + Ts z_k: Phi_a = [Phi 0; Ts C_z I], Gamma_a = [Gamma; Ts D_z]; the world's inputs and outputs."""
    Ts = _sampled(world, "dintegral_augmentation")
    iz, zl = _pick(z, world.y_labels, "an output", "dintegral_augmentation")
    k, nu = len(iz), world.nu
    integ = dintegrators_world(world.n, k, Ts, device)
    F = np.vstack([np.zeros((nu, k)), np.eye(k)])
    G = np.vstack([np.eye(nu), np.zeros((k, nu))])
    try:
        res = dconnect(world, integ, feedback=F, inputs=G, reads=iz, outputs=list(range(world.ny)), input_labels=world.u_labels)
    finally:
        integ.close()
    if not res.ok.all():
        bad = np.flatnonzero(~res.ok)
        res.world.close()
        raise FlightBatchError(f"dintegral_augmentation: dconnect flagged systems {bad.tolist()} (status {res.status[bad].tolist()})")
    aug = res.world
    aug.x_labels = tuple(world.x_labels) + tuple(f"ξ_{s}" for s in zl)
    return aug


def dlqr_tracker(world: LinearWorld, z, Q, R, Q_int=None, forward: str = "inverse", device: int = 0):
    """(K_fbk [N, nu, nx], K_fwd [N, nu, nz], K_int [N, nu, nz], status [N]) of the sampled tracker law, designed at the world's Ts: dlqr on
    the world (Q_int None: K_int = 0) or on its augmentation [x_k; ξ_k-1] (Q: the diagonal on x, Q_int: the diagonal on the integrators),
    K_aug = [K_x, K_ξ]. The flown integrator holds the current sample, ι_k = -K_int ξ_k, hence K_int = K_ξ and K_fbk = K_x - Ts K_ξ C_z; K_fwd
    = U + K_fbk X by dsteady_state (forward="inverse") or I (forward="identity"). With these gains the unbounded flown law is dlqr's optimal
    loop. status: dlqr's bits, or the map's shifted left by 8; a system with D_z != 0 under Q_int is flagged DIRECT << 8 and not designed."""
    _sampled(world, "dlqr_tracker")
    if forward not in ("inverse", "identity"):
        raise ValueError('dlqr_tracker: forward is "inverse" or "identity"')
    iz, _ = _pick(z, world.y_labels, "an output", "dlqr_tracker")
    nx, nz = world.nx, len(iz)
    if forward == "identity" and nz != world.nu:
        raise ValueError(f"dlqr_tracker: forward=\"identity\" takes as many z as inputs ({world.nu}), got {nz}")
    if Q_int is None:
        res = dlqr(world, Q, R)
        K_x, K_xi = res.K, None
    else:
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim != 1:
            raise ValueError("dlqr_tracker: with Q_int, Q is the diagonal on the states")
        aug = dintegral_augmentation(world, iz, device)
        try:
            res = dlqr(aug, np.concatenate([Q, np.asarray(Q_int, dtype=np.float64)]), R)
        finally:
            aug.close()
        K_x, K_xi = np.ascontiguousarray(res.K[:, :, :nx]), np.ascontiguousarray(res.K[:, :, nx:])
    good = (res.status == 0)[:, None, None]
    clean = lambda M: None if M is None else np.where(np.isfinite(M), M, 0.0)
    st = dsteady_state(world, iz, clean(K_x), clean(K_xi))
    K_fbk = np.where(good, st.K_fbk, np.nan)
    designed = np.isfinite(K_fbk).all(axis=(1, 2))[:, None, None]      # (neither dlqr nor the map flagged it)
    K_int = np.zeros((world.n, world.nu, nz)) if K_xi is None else np.where(designed, K_xi, np.nan)
    if forward == "identity":
        return K_fbk, np.where(designed, np.eye(nz)[None], np.nan), K_int, res.status | (st.status << 8)
    return K_fbk, np.where(good, st.K_fwd, np.nan), K_int, res.status | (st.status << 8)


def dtracker_world(world: LinearWorld, z, K_fbk, K_fwd, K_int, device: int = 0) -> LinearWorld:
    """the unbounded law closed around the sampled plant by dconnect: inputs z_ref, the plant's outputs, states [x; ι] (ι as it stands before
    a tick). For dpoles, timeresp.step and the next dconnect. The plant's output labels must include every state label (the law reads x
    from those rows, which are taken as the states themselves, as c172x_design_model's are) and D_z must be zero; gains [nu, .] for the batch or [N, nu, .] per system (all alike)."""
    Ts = _sampled(world, "dtracker_world")
    iz, zl = _pick(z, world.y_labels, "an output", "dtracker_world")
    n, nx, nu, nz = world.n, world.nx, world.nu, len(iz)
    missing = [s for s in world.x_labels if s not in world.y_labels]
    if missing:
        raise FlightBatchError(f"dtracker_world: the plant's outputs do not include its states {missing}: the law reads x from the outputs")
    ix = [world.y_labels.index(s) for s in world.x_labels]
    _, D = world.model_cd()
    if (D[:, iz, :] != 0.0).any():
        raise FlightBatchError("dtracker_world: D[z, :] has a non-zero entry: the law's delayed feed-through is not a dconnect of this plant (dtracker_metrics serves it)")
    per = [np.ndim(g) == 3 for g in (K_fbk, K_fwd, K_int)]
    if any(per) and not all(per):
        raise ValueError("dtracker_world: the three gains are all for the batch or all per system")
    lead = (n,) if per[0] else ()
    fbk, fwd, kin = (np.asarray(g, dtype=np.float64) for g in (K_fbk, K_fwd, K_int))
    for g, c, name in ((fbk, nx, "K_fbk"), (fwd, nz, "K_fwd"), (kin, nz, "K_int")):
        if g.shape != lead + (nu, c):
            raise ValueError(f"dtracker_world: {name} must be [{nu}, {c}] or [{n}, {nu}, {c}], got {g.shape}")
    # v = [u_p; e_ι], reads [x (nx); z (nz); ι_k (nu)]: u_p = -K_fbk x + ι_k + K_fwd z_ref, e_ι = K_int (z_ref - z)
    F = np.zeros(lead + (2 * nu, nx + nz + nu))
    G = np.zeros(lead + (2 * nu, nz))
    F[..., :nu, :nx] = -fbk
    F[..., :nu, nx + nz:] = np.eye(nu)
    F[..., nu:, nx:nx + nz] = -kin
    G[..., :nu, :] = fwd
    G[..., nu:, :] = kin
    integ = dintegrators_world(n, nu, Ts, device)
    try:
        res = dconnect(world, integ, feedback=F, inputs=G, reads=ix + [int(k) for k in iz] + list(range(world.ny, world.ny + nu)),
                       outputs=list(range(world.ny)), input_labels=tuple(f"{s}_ref" for s in zl))
    finally:
        integ.close()
    if not res.ok.all():
        bad = np.flatnonzero(~res.ok)
        res.world.close()
        raise FlightBatchError(f"dtracker_world: dconnect flagged systems {bad.tolist()} (status {res.status[bad].tolist()})")
    loop = res.world
    loop.x_labels = tuple(world.x_labels) + tuple(f"ι_{s}" for s in world.u_labels)
    return loop
