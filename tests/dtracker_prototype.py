"""The algorithm of fb_lss_dtracker_metrics restated in numpy fp64 (test infrastructure; kernel: csrc/dtracker_kernels.hpp;
docs/design/linearize.md, "Discrete LQR trackers on the device"), the exact side the tests hold both to, and the cases the CPU and GPU tests share.

    plant     Phi, Gamma, C_z, D_z of a sampled model;  pair K_fbk [nu, nx], K_fwd [nu, nz], K_int [nu, nz];  bounds lo < hi per input
    prototype the kernel's row layout: rows 0 .. nx - 1 are Phi_r with Gamma_r, the next nu rows K_fbk,j with K_int,j, the next nz rows C_z,c with
              D_z,c; one dot product of x_k per tick, summed over the columns in ascending order, serves all three kinds; then D_z u_k-1, K_int e,
              Gamma u_k, each summed in ascending index from the value the kernel starts from, the ONE law (lo = -Inf, hi = +Inf without
              bounds) and the trapezoids accumulated as f_0 / 2 + f_1 + ... + f_N / 2.
    exact     an independent, literal tick-by-tick transcription of the law as stated (FP/control.jl:708-743 with sat_ext = 0 and the trim
              values at the origin), one pair at a time, in matrix-vector products (law_exact). It shares nothing with the prototype's layout.
"""
import functools

import numpy as np

DIVERGED, NOT_FINITE, ROWS_MAX, DIRECT = 1, 2, 32, 4      # FB_DTRACK_*, FB_DSTEADY_DIRECT (include/flightbatch.h)
BLOWUP = 1e12
TS, T_SIM = 0.02, 2.0                                     # 100 ticks
N_TICKS = 100
# nx + nu + nz at every edge of the group sizes 8, 16 and 32
EDGES = {3: (1, 1, 1), 7: (4, 2, 1), 8: (4, 2, 2), 9: (5, 2, 2), 15: (9, 3, 3), 16: (12, 2, 2), 17: (11, 3, 3), 31: (15, 8, 8), 32: (16, 8, 8)}
N_REF, M_REF = 9, 5                                       # the pairs of an edge; BIG: the cases with 130 systems and with 64 candidates
BIG = ((9, 130, 5), (8, 3, 64))                           # (rows, n, m)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plants(nx, nu, nz, n, seed=11):
    """Phi [n, nx, nx], Gamma [n, nx, nu], C_z [n, nz, nx], D_z [n, nz, nu], zref [nz]: random maps scaled to a spectral radius that runs from
    0.5 to 1.02 over the batch (every fourth system unstable: 1.02^100 = 7.2 stays far from the blow-up bound), D_z = 0 on the even systems and
    random on the odd ones (read only)"""
    rng = np.random.default_rng(seed + 1000 * nx + 10 * nu + nz)
    Phi = rng.standard_normal((n, nx, nx))
    rho = np.abs(np.linalg.eigvals(Phi)).max(axis=1)
    want = np.where(np.arange(n) % 4 == 3, 1.02, 0.5 + 0.45 * rng.random(n))
    Phi *= (want / rho)[:, None, None]
    Gam = rng.standard_normal((n, nx, nu)) / np.sqrt(nx)
    Cz = rng.standard_normal((n, nz, nx)) / np.sqrt(nx)
    Dz = 0.1 * rng.standard_normal((n, nz, nu))
    Dz[0::2] = 0.0
    zref = np.round(0.5 + rng.random(nz), 3) * np.where(np.arange(nz) % 2 == 0, 1.0, -1.0)
    return frozen(Phi, Gam, Cz, Dz, zref)


@functools.lru_cache(maxsize=None)
def gains(nx, nu, nz, n, m, seed=12):
    """K_fbk [n, m, nu, nx], K_fwd, K_int [n, m, nu, nz]: small random gains (the loops need not track: the law's arithmetic is what is held)"""
    rng = np.random.default_rng(seed + 1000 * nx + 10 * nu + nz)
    Kfbk = 0.05 * rng.standard_normal((n, m, nu, nx)) / np.sqrt(nx)
    Kfwd = 0.5 * rng.standard_normal((n, m, nu, nz))
    Kint = 0.5 * rng.standard_normal((n, m, nu, nz))
    return frozen(Kfbk, Kfwd, Kint)


def pairs(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint):
    """the systems repeated along the candidates: [n m, ...] arrays, system index slowest"""
    m = Kfbk.shape[1]
    rep = lambda a: np.repeat(a, m, axis=0)
    flat = lambda a: a.reshape((-1,) + a.shape[2:])
    return rep(Phi), rep(Gam), rep(Cz), rep(Dz), flat(Kfbk), flat(Kfwd), flat(Kint)


def world(fb, Phi, Gam, Cz, Dz, seed=5, Ts=TS):
    """(sampled LinearWorld, z): the plants with nz + 2 outputs whose rows z = (nz, nz - 1, .., 1) carry C_z and D_z in reverse order, so the
    order of iz matters; the other rows, and delta, x0, u0, y0, are random numbers (they play no part)"""
    n, nx, nu = Gam.shape
    nz = Cz.shape[1]
    rng = np.random.default_rng(seed)
    iz = list(range(nz, 0, -1))
    C = rng.standard_normal((n, nz + 2, nx)); C[:, iz, :] = Cz
    D = rng.standard_normal((n, nz + 2, nu)); D[:, iz, :] = Dz
    lss = fb.LinearizedSS(xdot0=rng.standard_normal((n, nx)), x0=rng.standard_normal((n, nx)), u0=rng.standard_normal((n, nu)),
                          y0=rng.standard_normal((n, nz + 2)), A=Phi, B=Gam, C=C, D=D, x_labels=tuple(f"x{k}" for k in range(nx)),
                          u_labels=tuple(f"u{k}" for k in range(nu)), y_labels=tuple(f"y{k}" for k in range(nz + 2)))
    return fb.LinearWorld(lss, Ts=Ts), iz


# the bounded cases (D_z = 0): three lags driven by two inputs, an integrating tracker, eight pairs of bound sets
B_ZREF = np.array([1.0, -0.5])
B_BOUNDS = (((-np.inf, -np.inf), (0.3, np.inf)),          # input 0 clamps from above, input 1 is free: one input only
            ((-np.inf, -0.12), (np.inf, np.inf)),         # input 1 clamps from below only
            ((-0.4, -0.2), (0.4, 0.2)),                   # both clamp
            ((-0.35, -np.inf), (0.35, 0.5)),
            ((-5.0, -5.0), (5.0, 5.0)),                   # finite bounds that are never reached
            ((-np.inf, -np.inf), (np.inf, np.inf)),       # no bounds, written as infinities
            ((-0.25, -0.15), (0.25, 0.15)),
            ((-np.inf, -0.3), (0.45, np.inf)))


@functools.lru_cache(maxsize=None)
def bounded_cases():
    """Phi, Gam, Cz, Dz (zeros), Kfbk, Kfwd, Kint [n, m, ...], lo, hi [n, m, nu] with n = 3 plants and m = 8 bound sets (read only)"""
    n, m = 3, len(B_BOUNDS)
    Phi = np.array([[[0.90, 0.02, 0.0], [0.0, 0.85, 0.03], [0.01, 0.0, 0.8]]]) * np.array([1.0, 0.98, 1.03])[:, None, None]
    Gam = np.array([[[0.10, 0.0], [0.0, 0.12], [0.02, 0.02]]]) * np.array([1.0, 1.1, 0.9])[:, None, None]
    Cz = np.broadcast_to(np.array([[1.0, 0.0, 0.2], [0.0, 1.0, 0.0]]), (n, 2, 3)).copy()
    Dz = np.zeros((n, 2, 2))
    tile = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n, m) + np.shape(a)).copy()
    Kfbk = tile([[0.8, 0.0, 0.1], [0.0, 0.6, 0.0]])
    Kfwd = tile([[0.9, 0.0], [0.1, 0.7]])
    Kint = tile([[6.0, 0.0], [0.5, 5.0]])
    lo = np.broadcast_to(np.array([b[0] for b in B_BOUNDS])[None], (n, m, 2)).copy()
    hi = np.broadcast_to(np.array([b[1] for b in B_BOUNDS])[None], (n, m, 2)).copy()
    return frozen(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, lo, hi)


def failure_pairs():
    """the GPU test's failure pairs among healthy ones: six two-state plants, three candidates each (plant and gain arrays, expect [n, m]).
    System 2's candidate 1 feeds the state back with the wrong sign: Phi + 0.6 Gamma K has a pole at 1.5, and 1.5^100 > 1e12. System 4's
    candidate 0 has a NaN in K_int, candidate 2 an Inf in K_fwd."""
    n, m = 6, 3
    Phi, Gam, Cz, Dz, _ = (a.copy() for a in plants(2, 1, 1, n))
    Kfbk, Kfwd, Kint = (a.copy() for a in gains(2, 1, 1, n, m))
    Phi[2], Gam[2], Cz[2], Dz[2] = np.diag([0.9, 0.5]), np.array([[1.0], [0.0]]), np.array([[1.0, 0.0]]), 0.0
    Kfbk[2, 1] = np.array([[-0.6, 0.0]])
    Kint[4, 0, 0, 0] = np.nan
    Kfwd[4, 2, 0, 0] = np.inf
    expect = np.zeros((n, m), dtype=np.int32)
    expect[2, 1], expect[4, 0], expect[4, 2] = DIVERGED, NOT_FINITE, NOT_FINITE
    return Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, expect


# ---- the prototype ---------------------------------------------------------------------------------------------------------------------------------
def sample_rows(N, stride):
    """the ticks that come home: every stride-th and the last one (fb_lss_stepinfo_samples rows)"""
    ks = list(range(0, N + 1, stride))
    return np.array(ks if ks[-1] == N else ks + [N])


def tracker(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, zref, Ts, N, lo=None, hi=None):
    """what the kernel leaves for the pairs [B, ...]: dict(zs [B, nz, N + 1], us [B, nu, N + 1], zmet [B, nz, 3] (ie, ef, zp), umet [B, nu, 2]
    (iu, up), counts [B, nu, 2], status [B])"""
    B, nx, nu = Gam.shape
    nz = Cz.shape[1]
    lo = np.full((B, nu), -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full((B, nu), np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    rows = np.concatenate([Phi, Kfbk, Cz], axis=1)                    # [B, nx + nu + nz, nx]
    bad = ~np.array([all(np.isfinite(a[k]).all() for a in (Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint)) for k in range(B)])
    with np.errstate(all="ignore"):
        ff = np.zeros((B, nu))
        for c in range(nz):
            ff = Kfwd[:, :, c] * zref[c] + ff
        x, iota, sat, up = np.zeros((B, nx)), np.zeros((B, nu)), np.zeros((B, nu)), np.zeros((B, nu))
        se, su, zp, upk = np.zeros((B, nz)), np.zeros((B, nu)), np.zeros((B, nz)), np.zeros((B, nu))
        nsat, nhalt = np.zeros((B, nu), dtype=np.int32), np.zeros((B, nu), dtype=np.int32)
        blown = np.zeros(B, dtype=bool)
        zs, us = np.empty((B, nz, N + 1)), np.empty((B, nu, N + 1))
        for k in range(N + 1):
            v = np.zeros((B, nx + nu + nz))
            for col in range(nx):
                v = rows[:, :, col] * x[:, col:col + 1] + v
            z = v[:, nx + nu:]
            for j in range(nu):
                z = Dz[:, :, j] * up[:, j:j + 1] + z
            e = zref[None] - z
            vi = np.zeros((B, nu))
            for c in range(nz):
                vi = Kint[:, :, c] * e[:, c:c + 1] + vi
            halted = vi * sat > 0.0
            iota = np.where(halted, iota, Ts * vi + iota)
            fr = (iota + ff) - v[:, nx:nx + nu]
            u = np.where(fr == fr, np.minimum(np.maximum(fr, lo), hi), fr)
            sat = (fr >= hi).astype(float) - (fr <= lo).astype(float)
            xn = v[:, :nx]
            for j in range(nu):
                xn = Gam[:, :, j] * u[:, j:j + 1] + xn
            x, up = xn, u
            wk = 0.5 if k in (0, N) else 1.0
            se, su = wk * np.abs(e) + se, wk * np.abs(u) + su
            zp, upk = np.fmax(zp, np.abs(z)), np.fmax(upk, np.abs(u))
            last = np.abs(e)
            nsat += sat != 0.0
            nhalt += halted
            blown |= ~(np.abs(z) <= BLOWUP).all(axis=1) | ~(np.abs(u) <= BLOWUP).all(axis=1)
            zs[:, :, k], us[:, :, k] = z, u
    zmet, umet, counts = np.stack([se / N, last, zp], axis=2), np.stack([su / N, upk], axis=2), np.stack([nsat, nhalt], axis=2)
    status = np.where(bad, NOT_FINITE, np.where(blown, DIVERGED, 0)).astype(np.int32)
    flagged = status != 0
    zmet[flagged], umet[flagged], counts[flagged] = np.inf, np.inf, 0
    zmet[bad], umet[bad] = np.nan, np.nan
    return dict(zs=zs, us=us, zmet=zmet, umet=umet, counts=counts, status=status)


# ---- the exact side ----------------------------------------------------------------------------------------------------------------------------------
def law_exact(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, zref, Ts, N, lo=None, hi=None):
    """One pair, tick by tick, as the law is stated. Returns zs [nz, N + 1], us [nu, N + 1], counts [nu, 2] and the two smallest distances of the
    run: of free_k to a finite bound, over max(1, |bound|), and of an integrator's input to zero over the ticks that follow a clamped tick of
    that input (each +Inf where there is none)."""
    nx, nu = Gam.shape
    nz = Cz.shape[0]
    lo = np.full(nu, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(nu, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    x, u_prev, iota_prev, sat_prev = np.zeros(nx), np.zeros(nu), np.zeros(nu), np.zeros(nu)
    zs, us = np.empty((nz, N + 1)), np.empty((nu, N + 1))
    counts = np.zeros((nu, 2), dtype=np.int32)
    near, near_v = np.inf, np.inf
    with np.errstate(all="ignore"):
        for k in range(N + 1):
            z = Cz @ x + Dz @ u_prev
            int_in = Kint @ (zref - z)
            halted = int_in * sat_prev > 0
            iota = np.where(halted, iota_prev, iota_prev + Ts * int_in)
            free = iota + Kfwd @ zref - Kfbk @ x
            u = np.clip(free, lo, hi)
            sat = (free >= hi).astype(float) - (free <= lo).astype(float)
            for b in (lo, hi):
                fin = np.isfinite(b)
                if fin.any():
                    near = min(near, float((np.abs(free - b)[fin] / np.maximum(1.0, np.abs(b[fin]))).min()))
            if (sat_prev != 0).any():
                near_v = min(near_v, float(np.abs(int_in)[sat_prev != 0].min()))
            counts[:, 0] += sat != 0
            counts[:, 1] += halted
            zs[:, k], us[:, k] = z, u
            x = Phi @ x + Gam @ u
            u_prev, iota_prev, sat_prev = u, iota, sat
    return zs, us, counts, (near, near_v)


def metrics_of(zs, us, zref, N):
    """zmet [.., nz, 3] (ie, ef, zp), umet [.., nu, 2] (iu, up) from samples [.., rows, N + 1]"""
    fe, fu = np.abs(np.asarray(zref)[:, None] - zs), np.abs(us)
    trapz = lambda f: (0.5 * f[..., 0] + f[..., 1:N].sum(axis=-1) + 0.5 * f[..., N]) / N
    return np.stack([trapz(fe), fe[..., N], np.abs(zs).max(axis=-1)], axis=-1), np.stack([trapz(fu), fu.max(axis=-1)], axis=-1)


def exact(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, zref, Ts, N, lo=None, hi=None):
    """the prototype's dictionary (without status) on the exact side, and near [B, 2]"""
    B = Gam.shape[0]
    runs = [law_exact(Phi[k], Gam[k], Cz[k], Dz[k], Kfbk[k], Kfwd[k], Kint[k], zref, Ts, N, None if lo is None else lo[k], None if hi is None else hi[k])
            for k in range(B)]
    zs, us = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
    zmet, umet = metrics_of(zs, us, zref, N)
    return dict(zs=zs, us=us, zmet=zmet, umet=umet, counts=np.array([r[2] for r in runs])), np.array([r[3] for r in runs])


def design_form(Phi, Gam, Cz, K_aug, K_fwd, zref, Ts, N):
    """One pair (D_z = 0): the loop as dlqr designed it on the augmentation [x_k; xi_k-1], xi_k = xi_k-1 + Ts (z_k - zref):
    u_k = -K_x x_k - K_xi xi_k-1 + (K_fwd + Ts K_xi) zref. Returns zs [nz, N + 1], us [nu, N + 1]."""
    nx, nu = Gam.shape
    nz = Cz.shape[0]
    K_x, K_xi = K_aug[:, :nx], K_aug[:, nx:]
    x, xi = np.zeros(nx), np.zeros(nz)
    zs, us = np.empty((nz, N + 1)), np.empty((nu, N + 1))
    for k in range(N + 1):
        z = Cz @ x
        u = -K_x @ x - K_xi @ xi + (K_fwd + Ts * K_xi) @ zref
        zs[:, k], us[:, k] = z, u
        xi = xi + Ts * (z - zref)
        x = Phi @ x + Gam @ u
    return zs, us


def dsteady(Phi, Gam, Cz, Dz, K=None, K_xi=None, Ts=TS):
    """(X, U, K_fbk, K_fwd) of one system by numpy.linalg.solve"""
    nx, nu = Gam.shape
    L = np.block([[Phi - np.eye(nx), Gam], [Cz, Dz]])
    XU = np.linalg.solve(L, np.vstack([np.zeros((nx, nu)), np.eye(nu)]))
    X, U = XU[:nx], XU[nx:]
    if K is None:
        return X, U, None, None
    K_fbk = K if K_xi is None else K - Ts * K_xi @ Cz
    return X, U, K_fbk, U + K_fbk @ X


# ---- deviations ----------------------------------------------------------------------------------------------------------------------------------------
KEYS = ("zs", "us", "zmet", "umet")


def deviations(got, want):
    """per key: the samples' worst |got - want| over the largest |want| of that response, the metrics' worst |got - want| / |want|"""
    out = {}
    for k in ("zs", "us"):
        scale = np.abs(want[k]).max(axis=-1, keepdims=True)
        out[k] = float((np.abs(got[k] - want[k]) / scale).max())
    for k in ("zmet", "umet"):
        out[k] = float((np.abs(got[k] - want[k]) / np.abs(want[k])).max())
    return out


@functools.lru_cache(maxsize=None)
def edge_reference(rows, n=N_REF, m=M_REF):
    """the n x m pairs of one edge: plants, gains, zref, the prototype's and the exact side's dictionaries [n m, ...] (computed once, read only)"""
    nx, nu, nz = EDGES[rows]
    Phi, Gam, Cz, Dz, zref = plants(nx, nu, nz, n)
    Kfbk, Kfwd, Kint = gains(nx, nu, nz, n, m)
    args = pairs(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint)
    pro = tracker(*args, zref, TS, N_TICKS)
    ex, _ = exact(*args, zref, TS, N_TICKS)
    assert (pro["status"] == 0).all()
    for d in (pro, ex):
        frozen(*d.values())
    return Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, zref, pro, ex


@functools.lru_cache(maxsize=None)
def bounded_reference():
    """the bounded cases' prototype and exact dictionaries [n m, ...] and the exact side's distances near [n m, 2]"""
    Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, lo, hi = bounded_cases()
    args = pairs(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint)
    l, h = lo.reshape(-1, 2), hi.reshape(-1, 2)
    pro = tracker(*args, B_ZREF, TS, N_TICKS, l, h)
    ex, near = exact(*args, B_ZREF, TS, N_TICKS, l, h)
    assert (pro["status"] == 0).all()
    for d in (pro, ex):
        frozen(*d.values())
    return pro, ex, near


def take(d, n, m, n_ref=N_REF, m_ref=M_REF):
    """the first n systems and m candidates of a dictionary over n_ref x m_ref pairs, as [n, m, ...]"""
    return {k: v.reshape((n_ref, m_ref) + v.shape[1:])[:n, :m] for k, v in d.items()}


def flat(d):
    """[n, m, ...] -> [n m, ...] of such a dictionary"""
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in d.items()}
