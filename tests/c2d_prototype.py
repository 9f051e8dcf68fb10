"""The algorithms of fb_lss_c2d, of the sampled stepper and of the sampled fb_lss_stepinfo restated in numpy fp64, operation for operation (test
infrastructure; kernels: csrc/c2d_kernels.hpp, fbz::k_lss_map in csrc/lss_kernels.hpp, fbz::k_timeresp_map in csrc/timeresp_kernels.hpp;
docs/design/linearize.md, "Sampled models on the device"), the exact side the tests hold them to, and the cases of the GPU tests.

    the map     Psi = int_0^Ts e^(A tau) dtau;  Phi = e^(A Ts),  Gamma = Psi B,  delta = Psi xdot0;  x+ = x0 + Phi (x - x0) + Gamma (u - u0) + delta
    prototype   s = the smallest integer >= 0 with |A|_inf Ts / 2^s <= 1/2 (row sums over ascending columns), h = Ts / 2^s, Z = A h;
                S = I + (Z S) r_k for k = DEG .. 1 from S = I, r_k = 1 / (k + 1);  T = (S [B | xdot0]) h;  Phi = I + Z S;
                s times T <- T + Phi T, Phi <- Phi Phi; every product summed over ascending columns from its first accumulator (the kernel's
                fma is a multiplication and an addition here: the one difference)
    exact       scipy.linalg.expm of [[A, B, xdot0], [0]] Ts
"""
import numpy as np

import timeresp_prototype as tr

NOT_FINITE, RANGE, SQUARINGS_MAX = 1, 2, 30      # FB_C2D_* (include/flightbatch.h)
DEG = 16                                          # fbz::C2D_DEG
RK = [1.0 / (k + 1) for k in range(DEG + 1)]      # fbz::C2D_RK

# ---- the GPU tests' cases -----------------------------------------------------------------------------------------------------------------------
SEED = 73
NX_ALL = (1, 7, 8, 9, 16, 17, 31, 32)            # both sides of every group-size edge of k_lss_c2d
NU_ALL = (1, 8)
NY, N_SYS = 3, 9
TS_ALL = (1e-3, 0.02, 0.25)
FLOOR, MARGIN = 1e-11, 10.0                       # the family's rule (tests/test_gpu_timeresp.py)
NORM_MAX, PHI_MIN = 2.0 ** 8, 1e-3                # what makes a case fair: |A|_inf Ts <= 2^8 (s <= 9) and max|Phi| >= 1e-3
STEP_NX = (3, 7, 16, 31)                          # the sampled stepper's sizes: one per group size of k_lss_map (4, 8, 16, 32)
STEP_TS, STEP_N, STEP_EVERY = 0.02, 300, 100
SI_TS, SI_TSIM = tr.DT, tr.T_SIM                  # the sampled stepinfo runs tests/timeresp_prototype.py's pairs (NX_ALL, CHANNELS) at its dt


def plants(nx, nu, n=N_SYS, seed=SEED):
    """(xdot0, x0, u0, y0, A, B, C, D) [n, ...]: A = -(L L' + I / 2) + (S - S') with entries ~ N(0, 1 / nx) (the family's stable plants), the
    rest standard normal"""
    rng = np.random.default_rng(seed + 1000 * nx + nu)
    L = rng.standard_normal((n, nx, nx)) / np.sqrt(nx)
    S = rng.standard_normal((n, nx, nx)) / np.sqrt(nx)
    A = -(L @ L.transpose(0, 2, 1) + 0.5 * np.eye(nx)) + (S - S.transpose(0, 2, 1))
    B, Cm, D = rng.standard_normal((n, nx, nu)), rng.standard_normal((n, NY, nx)), rng.standard_normal((n, NY, nu))
    off = [rng.standard_normal((n, k)) for k in (nx, nx, nu, NY)]
    return (*off, A, B, Cm, D)


def scaled(nx, nu=1, factors=(1.0, 8.0, 64.0), n=N_SYS):
    """nine systems whose A is ONE plant times 1, 8, 64, 1, 8, ...: neighbouring groups of a wave square a different number of times"""
    M = [a[:1].repeat(n, axis=0) for a in plants(nx, nu, 1, SEED + 5)]
    f = np.array([factors[k % len(factors)] for k in range(n)])
    M[4] = M[4] * f[:, None, None]
    return tuple(M)


def model(fb, M, keep=slice(None)):
    xdot0, x0, u0, y0, A, B, Cm, D = (np.ascontiguousarray(b[keep]) for b in M)
    return fb.LinearizedSS(xdot0=xdot0, x0=x0, u0=u0, y0=y0, A=A, B=B, C=Cm, D=D, x_labels=tuple(f"x{k}" for k in range(A.shape[1])),
                           u_labels=tuple(f"u{k}" for k in range(B.shape[2])), y_labels=tuple(f"y{k}" for k in range(Cm.shape[1])))


# ---- c2d of one system ----------------------------------------------------------------------------------------------------------------------------
def row_times(X, W, acc):
    """acc + sum_c X[:, c] W[c, :], c ascending (every lane's row at once)"""
    for c in range(X.shape[1]):
        acc = acc + X[:, c:c + 1] * W[c:c + 1, :]
    return acc


def squarings_of(A, Ts):
    """(s, h) of the scaling: s stops one past SQUARINGS_MAX"""
    rs = np.zeros(A.shape[0])
    for c in range(A.shape[1]):
        rs = rs + np.abs(A[:, c])
    v, h, s = rs.max() * Ts, Ts, 0
    for _ in range(SQUARINGS_MAX + 1):
        if v > 0.5:
            v, h, s = 0.5 * v, 0.5 * h, s + 1
    return s, h


def c2d(A, B, xdot0, Ts):
    """(Phi [nx, nx], Gamma [nx, nu], delta [nx], s, status) of one system"""
    nx, nu = B.shape
    nan = (np.full((nx, nx), np.nan), np.full((nx, nu), np.nan), np.full(nx, np.nan), 0)
    if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(xdot0).all()):
        return (*nan, NOT_FINITE)
    with np.errstate(all="ignore"):
        s, h = squarings_of(A, Ts)
        if s > SQUARINGS_MAX:
            return (*nan, RANGE)
        Z, I = A * h, np.eye(nx)
        S = I.copy()
        for k in range(DEG, 0, -1):
            S = row_times(Z, S, np.zeros((nx, nx))) * RK[k] + I
        W = np.concatenate([B, xdot0[:, None]], axis=1)
        T = row_times(S, W, np.zeros((nx, nu + 1))) * h
        Phi = row_times(Z, S, I.copy())
        for _ in range(s):
            T = row_times(Phi, T, T.copy())
            Phi = row_times(Phi, Phi, np.zeros((nx, nx)))
    if not (np.isfinite(Phi).all() and np.isfinite(T).all()):
        return (*nan, NOT_FINITE)
    return Phi, T[:, :nu], T[:, nu], s, 0


def c2d_batch(A, B, xdot0, Ts):
    """(Phi [n, nx, nx], Gamma [n, nx, nu], delta [n, nx], s [n], status [n])"""
    out = [c2d(A[i], B[i], xdot0[i], Ts) for i in range(A.shape[0])]
    return tuple(np.array([o[k] for o in out]) for k in range(5))


def exact(A, B, xdot0, Ts):
    """(Phi, Gamma, delta) of one system from expm of the augmented [[A, B, xdot0], [0]] Ts"""
    from scipy.linalg import expm
    nx, nu = B.shape
    aug = np.zeros((nx + nu + 1, nx + nu + 1))
    aug[:nx, :nx], aug[:nx, nx:nx + nu], aug[:nx, nx + nu] = A, B, xdot0
    E = expm(aug * Ts)
    return E[:nx, :nx], E[:nx, nx:nx + nu], E[:nx, nx + nu]


def exact_batch(A, B, xdot0, Ts):
    out = [exact(A[i], B[i], xdot0[i], Ts) for i in range(A.shape[0])]
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def block_dev(got, want):
    """worst |got - want| of each system's block, scaled by the block's largest exact entry [n]"""
    n = want.shape[0]
    return np.abs(got - want).reshape(n, -1).max(axis=1) / np.abs(want).reshape(n, -1).max(axis=1)


def worst_dev(got3, want3):
    """the worst block_dev over Phi, Gamma and delta"""
    return max(float(block_dev(g, w).max()) for g, w in zip(got3, want3))


def fair(A, Phi_exact, Ts):
    """the two conditions on a GPU case: (|A|_inf Ts, max|Phi|) of one system"""
    return float(np.abs(A).sum(axis=1).max() * Ts), float(np.abs(Phi_exact).max())


# ---- the sampled stepper (fbz::k_lss_map) and the output record (fbl::k_lss_f_ode) -----------------------------------------------------------------
def map_steps(Phi, Gam, delta, x0, u0, x, u, nsteps):
    """nsteps of x <- x0 + (c0 + sum_c Phi[:, c] (x - x0)_c), c0 = delta + sum_c Gamma[:, c] (u - u0)_c, for a batch [n, ...]"""
    c0 = delta.copy()
    for c in range(Gam.shape[2]):
        c0 = c0 + Gam[:, :, c] * (u[:, c:c + 1] - u0[:, c:c + 1])
    for _ in range(nsteps):
        dx, acc = x - x0, c0.copy()
        for c in range(Phi.shape[2]):
            acc = acc + Phi[:, :, c] * dx[:, c:c + 1]
        x = x0 + acc
    return x


def outputs(Cm, D, x0, u0, y0, x, u):
    """y = y0 + C (x - x0) + D (u - u0), columns ascending [n, ny]"""
    acc, dx, du = y0.copy(), x - x0, u - u0
    for c in range(Cm.shape[2]):
        acc = acc + Cm[:, :, c] * dx[:, c:c + 1]
    for c in range(D.shape[2]):
        acc = acc + D[:, :, c] * du[:, c:c + 1]
    return acc


def lsim(Phi, Gam, delta, Cm, D, x0, u0, y0, x, U):
    """(y [nt, n, ny], x [nt, n, nx]) of the recursion under the inputs U [nt, n, nu], each held over its interval"""
    ys, xs = [], []
    for k in range(U.shape[0]):
        ys.append(outputs(Cm, D, x0, u0, y0, x, U[k]))
        xs.append(x)
        x = map_steps(Phi, Gam, delta, x0, u0, x, U[k], 1)
    return np.array(ys), np.array(xs)


# ---- the sampled stepinfo (fbz::k_timeresp_map): one dot product per sample; StepInfo itself is tests/timeresp_prototype.py's ------------------------
def samples_map(Phi, gam, c, d, N):
    """y [N + 1, B] of the pairs (Phi[k], gam[k], c[k], d[k]) from rest: y_k = d + c x_k, x_{k+1} = gam + Phi x_k"""
    B, nx = gam.shape
    x = np.zeros((B, nx))
    y = np.empty((N + 1, B))
    c3 = c[:, None, :]
    with np.errstate(all="ignore"):
        for k in range(N + 1):
            y[k] = tr._rows(c3, d[:, None], x)[:, 0]
            x = tr._rows(Phi, gam, x)
    return y


def stepinfo_case(nx):
    """the sampled stepinfo's case of one size: tests/timeresp_prototype.py's plants and channels; (plants, pairs of the prototype's sampled
    model, pairs of the exact sampled model)"""
    A, B, Cm, D = tr.plants(nx)
    z = np.zeros((A.shape[0], nx))
    Phi, Gam = c2d_batch(A, B, z, SI_TS)[:2]
    Phe, Gae = exact_batch(A, B, z, SI_TS)[:2]
    return (A, B, Cm, D), tr.pairs(Phi, Gam, Cm, D, tr.CHANNELS), tr.pairs(Phe, Gae, Cm, D, tr.CHANNELS)
