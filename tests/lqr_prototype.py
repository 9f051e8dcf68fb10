"""The algorithm of fb_lqr restated in numpy fp64, one system at a time (test infrastructure; kernels: csrc/lqr_kernels.hpp;
docs/design/linearize.md, "LQR design on the device"), and the generator of the random systems the LQR tests design.

    H = [[A, -G], [-Q, -A']], G = B inv(R) B'                     the Hamiltonian of the continuous-time Riccati equation
    Z <- (c Z + inv(Z) / c) / 2, c = |det Z|^(-1 / 2nx)           Newton's iteration for sign(H) with determinant scaling
    X = -W21 inv(I - W11), W = sign(H);  K = inv(R) B' X

inv(Z) is an in-place Gauss-Jordan elimination with partial pivoting done the way the kernel does it: the rows stay where they are
("lane r owns row r"), the pivot row of step k is the not yet used row with the largest |Z_ik| (ties: the lowest row), and the row and
column permutations are undone at the end. log|det| is the sum of the logs of the pivots of that elimination."""
import numpy as np

NOT_CONVERGED, SINGULAR = 1, 2      # FB_LQR_NOT_CONVERGED, FB_LQR_SINGULAR (include/flightbatch.h)
MAX_ITERS = 50
TOL = 1e-13

# (nx, nu) of the random systems (tests/test_lqr_host.py, tests/test_gpu_lqr.py)
SHAPES = [(1, 1), (2, 1), (3, 2), (4, 1), (5, 2), (8, 2), (9, 8), (11, 2), (16, 4)]
SEED = 11


def systems(nx, nu, n, seed=SEED):
    """A [n, nx, nx], B [n, nx, nu] per system; Q [nx, nx], R [nu, nu] one draw per shape"""
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((nx, nx)); M = rng.standard_normal((nu, nu))
    Q = L @ L.T / nx + 0.1 * np.eye(nx)
    R = M @ M.T / nu + 0.5 * np.eye(nu)
    A = rng.standard_normal((n, nx, nx)) / np.sqrt(nx)
    B = rng.standard_normal((n, nx, nu))
    return A, B, (Q + Q.T) / 2, (R + R.T) / 2


# the three systems without a stabilising solution (docs/design/linearize.md): (A, B, Q, R, status)
def failure_systems():
    return [
        (np.diag([1.0, -1.0]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1), SINGULAR),                   # unstable and uncontrollable
        (np.diag([0.0, -1.0]), np.array([[0.0], [1.0]]), np.diag([0.0, 1.0]), np.eye(1), SINGULAR),          # H is singular
        (np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]), np.array([[0.0], [0.0], [1.0]]),
         np.diag([0.0, 0.0, 1.0]), np.eye(1), NOT_CONVERGED),                                                # eigenvalues of H on the imaginary axis
    ]


def embed3(A, B, Q):
    """a 2-state system with a stable third state that nothing couples to (a 3-state one as it is)"""
    if A.shape[0] == 3:
        return A, B, Q
    A3 = -np.eye(3); A3[:2, :2] = A
    B3 = np.zeros((3, 1)); B3[:2] = B
    Q3 = np.eye(3); Q3[:2, :2] = Q
    return A3, B3, Q3


def gj_inverse(Z):
    """(inv(Z), log|det Z|, ok): in-place Gauss-Jordan with implicit row pivoting"""
    n = Z.shape[0]
    W = Z.copy()
    used = np.zeros(n, dtype=bool)
    sigma = np.zeros(n, dtype=int)      # the pivot row of step k
    logdet, ok = 0.0, True
    for k in range(n):
        v = np.where(used, -1.0, np.abs(W[:, k]))
        with np.errstate(invalid="ignore"):
            m = np.nanmax(v) if not np.all(np.isnan(v)) else np.nan
            cand = np.flatnonzero(~used & (v == m))
        if cand.size == 0 or not (m > 0.0) or not np.isfinite(m):
            ok = False
        p = int(cand[0]) if cand.size else k
        with np.errstate(all="ignore"):
            ip = 1.0 / W[p, k]
            row = W[p] * ip
            row[k] = ip
            f = W[:, k].copy()
            W -= np.outer(f, row)
            W[:, k] = -f * ip
            W[p] = row
            logdet += np.log(m)
        used[p] = True
        sigma[k] = p
    inv = np.empty_like(W)
    # W[sigma(i), j] = inv(Z)[i, sigma(j)]
    inv[np.ix_(np.arange(n), sigma)] = W[sigma]
    return inv, logdet, ok


def lqr(A, B, Q, R):
    """dict(K, X, resid, iters, status) of one system"""
    nx, nu = B.shape
    Rinv = np.linalg.inv(R)
    G = B @ Rinv @ B.T
    Z = np.block([[A, -G], [-Q, -A.T]])
    nan = dict(K=np.full((nu, nx), np.nan), X=np.full((nx, nx), np.nan), resid=np.nan)
    it, converged = 0, False
    while it < MAX_ITERS and not converged:
        it += 1
        inv, logdet, ok = gj_inverse(Z)
        with np.errstate(all="ignore"):
            c = np.exp(-logdet / (2 * nx))
            Zn = 0.5 * (c * Z + inv / c)
        if not ok or not np.all(np.isfinite(Zn)):
            return dict(nan, iters=it, status=SINGULAR)
        converged = np.abs(Zn - Z).max() <= TOL * np.abs(Zn).max()
        Z = Zn
    if not converged:
        return dict(nan, iters=it, status=NOT_CONVERGED)
    Minv, _, ok = gj_inverse(np.eye(nx) - Z[:nx, :nx])
    with np.errstate(all="ignore"):
        X = -Z[nx:, :nx] @ Minv
        X = 0.5 * (X + X.T)
        K = Rinv @ (B.T @ X)
        res = np.abs(A.T @ X + X @ A - X @ G @ X + Q).max() / max(np.abs(Q).max(), np.abs(X).max())
    if not ok or not (np.all(np.isfinite(X)) and np.all(np.isfinite(K))):
        return dict(nan, iters=it, status=SINGULAR)
    return dict(K=K, X=X, resid=res, iters=it, status=0)


def lqr_batch(A, B, Q, R):
    out = [lqr(A[i], B[i], Q, R) for i in range(A.shape[0])]
    return {k: np.array([o[k] for o in out]) for k in ("K", "X", "resid", "iters", "status")}


def scipy_lqr(A, B, Q, R):
    """(K, X) of one system from scipy's Schur solver: the yardstick"""
    from scipy.linalg import solve_continuous_are
    X = solve_continuous_are(A, B, Q, R)
    return np.linalg.solve(R, B.T @ X), X


def scipy_batch(A, B, Q, R):
    out = [scipy_lqr(A[i], B[i], Q, R) for i in range(A.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def rel_dev(got, want):
    """(on purpose not support.state_scale: gains and Riccati solutions have no state rows) worst |got - want| / max|want| over the systems of a batch, each system scaled by its own largest entry"""
    axes = tuple(range(1, want.ndim))
    return float((np.abs(got - want).max(axis=axes) / np.abs(want).max(axis=axes)).max())
