"""The algorithm of fb_lss_dpid_metrics restated in numpy fp64 (test infrastructure; kernel: csrc/dpid_kernels.hpp; docs/design/linearize.md,
"Discrete PID design on the device"), the exact side the tests hold both to, and the cases the CPU and GPU tests share.

    plant     Phi, gamma, c, d of one channel of a sampled model;  point p = (k_p, k_i, k_d, tau_f), alpha = 1 / (tau_f + Ts);  bounds lo < hi
    prototype the kernel's row layout: rows 0 .. nx - 1 are Phi_r with gamma_r, row nx is c; one dot product of x_k per tick, summed over the
              columns in ascending order, is Phi_r x_k on the state rows and s_k on row nx; then the law, x_k+1,r = gamma_r u_k + Phi_r x_k, and
              the trapezoids accumulated as f_0 / 2 + f_1 + ... + f_N / 2. P(z) by complex Gauss-Jordan elimination with the kernel's pivot
              rule (pid_prototype.gj_solve) on z = cos + j sin, C(z) written out as the kernel writes it.
    exact     an independent, literal tick-by-tick transcription of the law as a scalar loop around Phi @ x (law_exact), P(z) by
              np.linalg.solve and C(z) in complex arithmetic from z = exp(j w Ts) (ms_exact). It shares nothing with the prototype's layout.
"""
import functools

import numpy as np

import pid_prototype as pp

DIVERGED, SINGULAR, DIRECT, NX_MAX = 1, 2, 4, 31      # FB_DPID_* (include/flightbatch.h)
MS_MAX, BLOWUP = 1e3, 1e12
TS, T_SIM = 0.02, 2.0                                  # 100 ticks
NX_EDGES = (1, 7, 8, 15, 16, 31)                       # nx + 1 straddles the group sizes 8, 16 and 32
N_REF, M_REF = 130, 5


def W7(Ts=TS):
    """seven frequencies up to the Nyquist frequency"""
    return np.logspace(-3.0, 0.0, 7) * (np.pi / Ts) * (1.0 - 1e-12)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def zoh(A, b, Ts):
    """Phi [n, nx, nx], gamma [n, nx]: the zero-order hold of x' = A x + b u by scipy's expm of the augmented matrix"""
    from scipy.linalg import expm
    n, nx = b.shape
    M = np.zeros((n, nx + 1, nx + 1))
    M[:, :nx, :nx] = A
    M[:, :nx, nx] = b
    E = np.array([expm(M[k] * Ts) for k in range(n)])
    return E[:, :nx, :nx].copy(), E[:, :nx, nx].copy()


@functools.lru_cache(maxsize=None)
def dplants(nx, n, Ts=TS):
    """Phi, gamma, c, d of the zero-order hold at Ts of pid_prototype.plants(nx, n): passive plants, d alternating 0 and 0.05 (read only)"""
    A, b, c, d = pp.plants(nx, n)
    Phi, gam = zoh(A, b, Ts)
    out = (Phi, gam, c.copy(), d.copy())
    for a in out:
        a.setflags(write=False)
    return out


def dpoints(n, m):
    """pid_prototype.points with tau_f in [0.02, 0.1], except that every third pair has tau_f = 0 (the plain backward difference) and every
    third, offset by one, tau_f = Ts / 2 (the stored q2e gains' ratio)"""
    P = pp.points(n, m).copy()
    flat = P.reshape(-1, 4)
    flat[0::3, 3] = 0.0
    flat[1::3, 3] = TS / 2
    return P


def model(fb, Phi, gam, c, d, Ts=TS):
    """the plants as a one-input, one-output sampled LinearWorld"""
    return fb.LinearWorld(pp.model(fb, Phi, gam, c, d), Ts=Ts)


# the bounded cases (d = 0): the family's passive plants at nx = 3, two gain sets under five pairs of bounds each
B_NX, B_N = 3, 4
B_GAINS = ((2.0, 6.0, 0.05, 0.01), (4.0, 10.0, 0.1, 0.02))
B_BOUNDS = ((-1.2, 1.2), (-1.5, 1.5), (-2.0, 2.0), (-3.0, 3.0), (-np.inf, 1.4))


@functools.lru_cache(maxsize=None)
def bounded_cases():
    """Phi, gamma, c, d (zeros), P [n, m, 4], lo, hi [n, m] with m = 10: candidate j has gains j // 5 and bounds j % 5"""
    Phi, gam, c, _ = dplants(B_NX, B_N)
    m = len(B_GAINS) * len(B_BOUNDS)
    P = np.array([B_GAINS[j // len(B_BOUNDS)] for j in range(m)])
    lo = np.array([B_BOUNDS[j % len(B_BOUNDS)][0] for j in range(m)])
    hi = np.array([B_BOUNDS[j % len(B_BOUNDS)][1] for j in range(m)])
    tile = lambda a: np.broadcast_to(a[None], (B_N,) + a.shape).copy()
    out = (Phi, gam, c, np.zeros(B_N), tile(P), tile(lo), tile(hi))
    for a in out:
        a.setflags(write=False)
    return out


def failure_pairs():
    """the GPU test's failure pairs among healthy ones: seven one-state plants, three candidates each (Phi, gam, c, d, P, lo, hi, expect)"""
    n, m = 7, 3
    Phi, gam, c, d = (a.copy() for a in dplants(1, n))
    P = dpoints(n, m)
    lo, hi = np.full((n, m), -np.inf), np.full((n, m), np.inf)
    Phi[2], gam[2], c[2], d[2] = 1.5, 1.0, 1.0, 0.0                      # a pole at z = 1.5
    P[2] = np.array([0.9, 0.0, 0.0, 0.01]); P[2, 1] = np.array([0.1, 0.0, 0.0, 0.01])      # loop pole 1.5 - k_p: 0.6, and 1.4: 1.4^100 > 1e12
    Phi[5], gam[5], c[5], d[5] = 0.5, 1.0, 1.0, -0.5
    P[5] = np.array([0.5, 0.5, 0.0, 0.01]); P[5, 0] = np.array([2.0, 0.0, 0.0, 0.01])      # d Dc = -1 exactly
    lo[3, 2], hi[3, 2] = -2.0, 2.0                                       # system 3 has d = 0.05: a finite bound on it
    hi[4, 1] = 1.5                                                       # system 4 has d = 0: a healthy bounded pair
    expect = np.zeros((n, m), dtype=np.int32)
    expect[2, 1], expect[5, 0], expect[3, 2] = DIVERGED, SINGULAR, DIRECT
    return Phi, gam, c, d, P, lo, hi, expect


# ---- the prototype ---------------------------------------------------------------------------------------------------------------------------------
def c_response(p, Ts, cs, sn):
    """C(z) on z = cs + j sn, written out as the kernel does: z / (z - 1) = ((1 - cos) - j sin) / |.|^2, (z - 1) / (z - q) with q = alpha tau_f"""
    kp, ki, kd, tf = p
    al = 1.0 / (tf + Ts)
    ar = 1.0 - cs
    im2 = ar * ar + sn * sn
    qr = cs - al * tf
    qm2 = qr * qr + sn * sn
    dr, di = (-ar * qr + sn * sn) / qm2, (sn * qr + ar * sn) / qm2
    return (kp + Ts * ki * (ar / im2) + al * kd * dr) + 1j * (al * kd * di - Ts * ki * (sn / im2))


def dfreqresp(Phi, gam, c, d, cs, sn):
    """P(z) [nw] of one plant by the kernel's elimination; NaN where a pivot was zero or not finite"""
    nx = Phi.shape[0]
    out = np.empty(len(cs), dtype=complex)
    for j in range(len(cs)):
        x, ok = pp.gj_solve((cs[j] + 1j * sn[j]) * np.eye(nx) - Phi, gam)
        val = d + np.sum(c * x)
        out[j] = val if ok and np.isfinite(val) else np.nan
    return out


def time_metrics(Phi, gam, c, d, P, lo, hi, Ts, N):
    """what the kernel's tick loop leaves for the pairs (Phi[k], gam[k], c[k], d[k]; P[k], lo[k], hi[k]): (ie, ef, iu, up) [B, 4], the
    blow-up flag [B] and the counts [B, 2]"""
    B, nx = gam.shape
    rows = np.concatenate([Phi, c[:, None, :]], axis=1)              # [B, nx + 1, nx]
    kp, ki, kd, tf = P.T
    al = 1.0 / (tf + Ts)
    alkd, altf, tski = al * kd, al * tf, Ts * ki
    tsalkd = Ts * alkd
    Dc = kp + tski + alkd
    bounded = np.isfinite(lo) | np.isfinite(hi)
    with np.errstate(all="ignore"):
        gg = 1.0 / (1.0 + d * Dc)
        x = np.zeros((B, nx))
        xi, eta, sat = np.zeros(B), np.zeros(B), np.zeros(B)
        sy, su, peak, last = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
        nsat, nhalt = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        blown = np.zeros(B, dtype=bool)
        for k in range(N + 1):
            v = np.zeros((B, nx + 1))
            for col in range(nx):
                v = v + rows[:, :, col] * x[:, col:col + 1]
            s = v[:, nx]
            one_s = 1.0 - s
            # a pair with a finite bound
            halted = bounded & (one_s * sat > 0.0)
            xi_b = np.where(halted, xi, tski * one_s + xi)
            fr = (kp * one_s + xi_b) + al * (kd * one_s - eta)
            u_b = np.where(fr == fr, np.minimum(np.maximum(fr, lo), hi), fr)
            sat_b = (fr >= hi).astype(float) - (fr <= lo).astype(float)
            # a pair without
            u_u = gg * ((Dc * one_s + xi) - al * eta)
            e_u = one_s - d * u_u
            u = np.where(bounded, u_b, u_u)
            e = np.where(bounded, one_s, e_u)
            xi = np.where(bounded, xi_b, tski * e_u + xi)
            sat = np.where(bounded, sat_b, 0.0)
            nsat += (sat != 0.0)
            nhalt += halted
            eta = altf * eta + tsalkd * e
            y = d * u + s
            x = gam * u[:, None] + v[:, :nx]
            fy, fu = np.abs(y - 1.0), np.abs(u - 1.0)
            wk = 0.5 if k in (0, N) else 1.0
            sy, su = sy + wk * fy, su + wk * fu
            peak = np.fmax(peak, fu)
            last = fy
            blown |= ~(np.abs(y) <= BLOWUP) | ~(np.abs(u) <= BLOWUP)
    return np.stack([sy / N, last, su / N, peak], axis=1), blown, np.stack([nsat, nhalt], axis=1)


def metrics(Phi, gam, c, d, P, w, Ts, N, lo=None, hi=None, weights=None):
    """metrics [B, 5] (Ms, ie, ef, iu, up), cost [B], status [B], counts [B, 2] of the pairs, the kernel's way"""
    B = P.shape[0]
    lo = np.full(B, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(B, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    wt = np.ones(5) if weights is None else np.asarray(weights, dtype=np.float64)
    cs, sn = np.cos(w * Ts), np.sin(w * Ts)
    tm, blown, counts = time_metrics(Phi, gam, c, d, P, lo, hi, Ts, N)
    out, cost, status = np.empty((B, 5)), np.empty(B), np.zeros(B, dtype=np.int32)
    cache = {}
    for k in range(B):
        key = (Phi[k].tobytes(), gam[k].tobytes(), c[k].tobytes(), float(d[k]))
        if key not in cache:
            cache[key] = dfreqresp(Phi[k], gam[k], c[k], d[k], cs, sn)
        pw = cache[key]
        bounded = np.isfinite(lo[k]) or np.isfinite(hi[k])
        with np.errstate(all="ignore"):
            al = 1.0 / (P[k, 3] + Ts)
            den = 1.0 + d[k] * (P[k, 0] + Ts * P[k, 1] + al * P[k, 2])
            sing = (not bounded and (den == 0.0 or not np.isfinite(1.0 / den))) or not np.all(np.isfinite(pw))
        if bounded and d[k] != 0.0:
            status[k], out[k], cost[k], counts[k] = DIRECT, np.nan, np.inf, 0
            continue
        if sing:
            status[k], out[k], cost[k], counts[k] = SINGULAR, np.nan, np.inf, 0
            continue
        with np.errstate(all="ignore"):
            L = pw * c_response(P[k], Ts, cs, sn)
            out[k, 0] = min(float(np.max(1.0 / np.abs(1.0 + L))), MS_MAX)
        if blown[k]:
            status[k], out[k, 1:], cost[k] = DIVERGED, np.inf, np.inf
            continue
        out[k, 1:] = tm[k]
        cost[k] = np.sum(wt * out[k]) / np.sum(wt)
    return out, cost, status, counts


# ---- the exact side ----------------------------------------------------------------------------------------------------------------------------------
def law_exact(Phi, gam, c, d, p, Ts, N, lo=-np.inf, hi=np.inf):
    """One pair, tick by tick, as the law is stated. Returns y, u [N + 1], the two counts, and the smallest distances of the run: of free_k
    to a bound over all ticks, and of e_k to zero over the ticks that follow a clamped tick (both +Inf for an unbounded pair)."""
    kp, ki, kd, tf = (float(v) for v in p)
    alpha = 1.0 / (tf + Ts)
    x = np.zeros(len(gam))
    xi_prev, eta_prev, sat_prev = 0.0, 0.0, 0
    ys, us = np.empty(N + 1), np.empty(N + 1)
    n_sat = n_halt = 0
    near_bound = near_zero = np.inf
    finite_bound = np.isfinite(lo) or np.isfinite(hi)
    for k in range(N + 1):
        s = float(c @ x)
        if finite_bound:
            e = 1.0 - s
            halted = e * sat_prev > 0
            xi = xi_prev if halted else xi_prev + Ts * ki * e
            free = kp * e + xi + alpha * (kd * e - eta_prev)
            u = min(max(free, lo), hi)
            sat = int(free >= hi) - int(free <= lo)
            near_bound = min(near_bound, abs(free - lo), abs(free - hi))
            if sat_prev != 0:
                near_zero = min(near_zero, abs(e))
            n_sat += sat != 0
            n_halt += bool(halted)
        else:
            D_c = kp + Ts * ki + alpha * kd
            u = (D_c * (1.0 - s) + xi_prev - alpha * eta_prev) / (1.0 + d * D_c)
            e = 1.0 - s - d * u
            xi = xi_prev + Ts * ki * e
            sat = 0
        eta = alpha * tf * eta_prev + Ts * alpha * kd * e
        ys[k], us[k] = s + d * u, u
        x = Phi @ x + gam * u
        xi_prev, eta_prev, sat_prev = xi, eta, sat
    return ys, us, (n_sat, n_halt), (near_bound, near_zero)


def ms_exact(Phi, gam, c, d, p, w, Ts):
    kp, ki, kd, tf = p
    alpha = 1.0 / (tf + Ts)
    z = np.exp(1j * w * Ts)
    nx = Phi.shape[0]
    Pz = np.array([d + c @ np.linalg.solve(zz * np.eye(nx) - Phi, gam.astype(complex)) for zz in z])
    Cz = kp + ki * Ts * z / (z - 1.0) + kd * alpha * (z - 1.0) / (z - alpha * tf)
    return min(float(np.max(1.0 / np.abs(1.0 + Pz * Cz))), MS_MAX)


def exact(Phi, gam, c, d, P, w, Ts, N, lo=None, hi=None):
    """metrics [B, 5], counts [B, 2] and the two smallest distances [B, 2] of the pairs on the exact side (healthy pairs only)"""
    B = P.shape[0]
    out, counts, near = np.empty((B, 5)), np.empty((B, 2), dtype=np.int32), np.empty((B, 2))
    for k in range(B):
        y, u, counts[k], near[k] = law_exact(Phi[k], gam[k], c[k], d[k], P[k], Ts, N, -np.inf if lo is None else lo[k], np.inf if hi is None else hi[k])
        fy, fu = np.abs(y - 1.0), np.abs(u - 1.0)
        trapz = lambda f: (0.5 * f[0] + f[1:N].sum() + 0.5 * f[N]) / N
        out[k] = ms_exact(Phi[k], gam[k], c[k], d[k], P[k], w, Ts), trapz(fy), fy[N], trapz(fu), fu.max()
    return out, counts, near


def closed_loop(Phi, gam, c, d, ctl):
    """the unbounded loop of one pair as ONE sampled model from r to (y, u, e): the compensator ctl = (Phi_c, Gamma_c, C_c, D_c) (build_dpid)
    in negative unity feedback around the plant, the algebraic loop through d solved. Returns Phi_l [nz, nz], Gamma_l [nz, 1], C_l [3, nz],
    D_l [3, 1] with z = (x, x_c)."""
    Pc, Gc, Cc, Dc = ctl
    nx, nc = len(gam), Pc.shape[0]
    g = 1.0 / (1.0 + d * Dc[0, 0])
    urow = g * np.concatenate([-Dc[0, 0] * c, Cc[0]])                 # u = urow z + uc r
    uc = g * Dc[0, 0]
    yrow = np.concatenate([c, np.zeros(nc)]) + d * urow               # y = c x + d u
    yc = d * uc
    M = np.zeros((nx + nc, nx + nc))
    M[:nx, :nx] = Phi
    M[nx:, nx:] = Pc
    M[:nx] += np.outer(gam, urow)
    M[nx:] += np.outer(Gc[:, 0], -yrow)                               # e = r - y
    v = np.concatenate([gam * uc, Gc[:, 0] * (1.0 - yc)])
    return M, v[:, None], np.stack([yrow, urow, -yrow]), np.array([[yc], [uc], [1.0 - yc]])


def host_metrics(y, u, S, N):
    """(Ms, ie, ef, iu, up) from samples y, u [N + 1] and the sensitivity S [nw] on the grid"""
    fy, fu = np.abs(y - 1.0), np.abs(u - 1.0)
    trapz = lambda f: (0.5 * f[0] + f[1:N].sum() + 0.5 * f[N]) / N
    return np.array([min(float(np.abs(S).max()), MS_MAX), trapz(fy), fy[N], trapz(fu), fu.max()])


rel_dev = pp.rel_dev


def pairs(Phi, gam, c, d, P):
    """the systems repeated along the candidates: ([n m, ...] plant arrays, P [n m, 4]), system index slowest"""
    m = P.shape[1]
    rep = lambda a: np.repeat(a, m, axis=0)
    return rep(Phi), rep(gam), rep(c), rep(d), P.reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def edge_reference(nx):
    """the N_REF x M_REF pairs of one nx: plants, points, the prototype's and the exact side's metrics [N_REF, M_REF, 5] (computed once, read only)"""
    Phi, gam, c, d = dplants(nx, N_REF)
    P = dpoints(N_REF, M_REF)
    args = pairs(Phi, gam, c, d, P)
    N = int(round(T_SIM / TS))
    pro, _, st, _ = metrics(*args, W7(), TS, N)
    ex, _, _ = exact(*args, W7(), TS, N)
    assert (st == 0).all()
    out = (Phi, gam, c, d, P, pro.reshape(N_REF, M_REF, 5), ex.reshape(N_REF, M_REF, 5))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bounded_reference():
    """the bounded cases with the prototype's and the exact side's metrics [n, m, 5], counts [n, m, 2] and the exact side's distances [n, m, 2]"""
    Phi, gam, c, d, P, lo, hi = bounded_cases()
    n, m = lo.shape
    args = pairs(Phi, gam, c, d, P)
    N = int(round(T_SIM / TS))
    pro, _, st, pc = metrics(*args, W7(), TS, N, lo.reshape(-1), hi.reshape(-1))
    ex, ec, near = exact(*args, W7(), TS, N, lo.reshape(-1), hi.reshape(-1))
    assert (st == 0).all()
    out = (pro.reshape(n, m, 5), pc.reshape(n, m, 2), ex.reshape(n, m, 5), ec.reshape(n, m, 2), near.reshape(n, m, 2))
    for a in out:
        a.setflags(write=False)
    return out
