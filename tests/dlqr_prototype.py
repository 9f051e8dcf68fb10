"""The algorithm of fb_lss_dlqr restated in numpy fp64, one system at a time, operation for operation (test infrastructure; kernel:
csrc/dlqr_kernels.hpp; docs/design/linearize.md, "Discrete LQR on the device"), the yardstick the tests hold it to, and the cases of the GPU
tests.

    the equation   X = Phi' X Phi - Phi' X Gam inv(R + Gam' X Gam) Gam' X Phi + Q,   K = inv(R + Gam' X Gam) Gam' X Phi
    doubling       A = Phi, G = Gam inv(R) Gam', H = Q;   W = I + G H,  [V | U] = inv(W) [A | G]  (one solve with the family's pivot rule)
                   H <- H + A' (H V),  G <- G + (A U) A',  A <- A V
                   until max|dH| <= TOL max|H| and max|A| <= A_TOL (at most MAX_ITERS doublings): A_k is the closed loop over 2^k samples
    the gain       X = (H + H') / 2;  Phic = inv(I + G0 X) Phi (the closed loop, the same solve);  K = inv(R) (Gam' (X Phic))
    the residual   max|Phi' (X (Phi - Gam K)) - X + Q| / max(max|Q|, max|X|)

Every product is summed over ascending columns from its first accumulator (the kernel's fma is a multiplication and an addition here: the
one difference). The solve is tests/surgery_prototype.py's, the numpy restatement of fbg::gj_solve."""
import numpy as np

import c2d_prototype as c2d
import lqr_prototype as lq
from surgery_prototype import solve

NOT_CONVERGED, SINGULAR = 1, 2      # FB_DLQR_NOT_CONVERGED, FB_DLQR_SINGULAR (include/flightbatch.h)
MAX_ITERS, NX_MAX = 40, 16          # FB_DLQR_MAX_ITERS, FB_DLQR_NX_MAX
TOL, A_TOL = 1e-13, 2.0 ** -20      # fbk::DLQR_TOL, fbk::DLQR_A_TOL

# ---- the GPU tests' cases -------------------------------------------------------------------------------------------------------------------------
SHAPES = lq.SHAPES
TS_ALL = (0.02, 0.25)
NMAX = 130
FLOOR, MARGIN, RESID_FLOOR = 1e-11, 10.0, 1e-13
DECISION_MIN = 1.01      # how far, as a factor, every deciding quantity of a doubling has to stay from its threshold (tests/test_dlqr_host.py)
COST_SHAPES, COST_TS, COST_N = ((3, 2), (8, 2), (16, 4)), 0.25, 9
LIMIT_TS = (0.02, 0.01, 0.005)


N_DISTINCT = 9


def batch(nx, nu, n):
    """(A [n, nx, nx], B [n, nx, nu], Q, R): tests/lqr_prototype.py's systems(nx, nu, 9), the nine systems per shape the recursion was first
    checked on, repeated in order up to n. Not systems(nx, nu, n): among its 130 draws are systems on which the yardstick itself
    is off (scipy.linalg.solve_discrete_are leaves a residual of 4.6e-9 on system 54 of (4, 1), 1.1e-10 on 118 of (11, 2); the doubling
    leaves 2.5e-12 and 6.5e-13 there), so a deviation from it would say nothing. tests/test_dlqr_host.py asserts that these nine are
    fair at both sample times. The bitwise tests, which need no yardstick, do run 130 distinct systems."""
    A, B, Q, R = lq.systems(nx, nu, N_DISTINCT)
    idx = np.arange(n) % N_DISTINCT
    return A[idx], B[idx], Q, R


def sampled(nx, nu, n, Ts):
    """(A, B, Phi, Gam, Q, R): the systems of one shape and their zero-order-hold models from the c2d prototype"""
    A, B, Q, R = batch(nx, nu, n)
    Phi, Gam, _, _, st = c2d.c2d_batch(A, B, np.zeros((n, nx)), Ts)
    assert (st == 0).all()
    return A, B, Phi, Gam, Q, R


def failure_case(Ts=0.25):
    """(A [66, 3, 3], B [66, 3, 1], Q, R, where, statuses): 66 (3, 1) systems, 5, 64 and 65 replaced by lqr_prototype's three systems
    without a stabilising solution, embedded as test_gpu_lqr.py embeds them; Q = diag(0, 0, 1), R = 1"""
    A, B, _, _ = lq.systems(3, 1, 66)
    A, B = A.copy(), B.copy()
    where = (5, 64, 65)
    for i, (a, b, q, _, _) in zip(where, lq.failure_systems()):
        A[i], B[i], _ = lq.embed3(a, b, q)
    return A, B, np.diag([0.0, 0.0, 1.0]), np.eye(1), where, (SINGULAR, NOT_CONVERGED, NOT_CONVERGED)


# ---- the algorithm --------------------------------------------------------------------------------------------------------------------------------
def row_times(X, W, acc):
    """acc + sum_c X[:, c] W[c, :], c ascending (every lane's row at once)"""
    for c in range(X.shape[1]):
        acc = acc + X[:, c:c + 1] * W[c:c + 1, :]
    return acc


def g_of(Gam, Rinv):
    """G0 = (Gam inv(R)) Gam': y_ra = sum_b Gam_rb Rinv_ba, G_rj = sum_a y_ra Gam_ja"""
    return row_times(row_times(Gam, Rinv, np.zeros_like(Gam)), Gam.T, np.zeros((Gam.shape[0],) * 2))


def _apart(v, th):
    """how far a deciding quantity is from its threshold, as a factor >= 1 (inf when either is zero)"""
    return max(v / th, th / v) if v > 0.0 and th > 0.0 else np.inf


def dlqr(Phi, Gam, Q, R):
    """dict(K, X, resid, iters, status) of one system; a designed one also has `margin`: the smallest factor by which a deciding quantity
    of a doubling (max|dH| against TOL max|H|, max|A| against A_TOL) missed its threshold, on either side. The count of doublings of
    another rounding of the same arithmetic is the same unless that factor is within rounding of 1."""
    nx, nu = Gam.shape
    nan = dict(K=np.full((nu, nx), np.nan), X=np.full((nx, nx), np.nan), resid=np.nan)
    Rinv = np.linalg.inv(R)
    I = np.eye(nx)
    with np.errstate(all="ignore"):
        A, G0, H = Phi.copy(), g_of(Gam, Rinv), Q.copy()
        G = G0.copy()
        it, converged, margin = 0, False, np.inf
        while it < MAX_ITERS and not converged:
            it += 1
            W = row_times(G, H, I.copy())
            VU, ok, _ = solve(W, np.concatenate([A, G], axis=1))
            V, U = VU[:, :nx], VU[:, nx:]
            Hn = row_times(A.T, row_times(H, V, np.zeros((nx, nx))), H.copy())
            Gn = row_times(row_times(A, U, np.zeros((nx, nx))), A.T, G.copy())
            An = row_times(A, V, np.zeros((nx, nx)))
            if not ok or not (np.isfinite(An).all() and np.isfinite(Gn).all() and np.isfinite(Hn).all()):
                return dict(nan, iters=it, status=SINGULAR)
            dh, hmax, amax = np.abs(Hn - H).max(), np.abs(Hn).max(), np.abs(An).max()
            converged = bool(dh <= TOL * hmax and amax <= A_TOL)
            margin = min(margin, _apart(dh, TOL * hmax), _apart(amax, A_TOL))
            A, G, H = An, Gn, Hn
        if not converged:
            return dict(nan, iters=it, status=NOT_CONVERGED)
        X = 0.5 * (H + H.T)
        Phic, ok, _ = solve(row_times(G0, X, I.copy()), Phi)
        S = row_times(X, Phic, np.zeros((nx, nx)))
        K = row_times(Rinv, row_times(Gam.T, S, np.zeros((nu, nx))), np.zeros((nu, nx)))
        Pcl = row_times(-Gam, K, Phi.copy())
        E = (row_times(Phi.T, row_times(X, Pcl, np.zeros((nx, nx))), np.zeros((nx, nx))) - X) + Q
        res = np.abs(E).max() / max(np.abs(Q).max(), np.abs(X).max())
    if not ok or not (np.isfinite(K).all() and np.isfinite(res)):
        return dict(nan, iters=it, status=SINGULAR)
    return dict(K=K, X=X, resid=res, iters=it, status=0, margin=margin)


def dlqr_batch(Phi, Gam, Q, R):
    out = [dlqr(Phi[i], Gam[i], Q, R) for i in range(Phi.shape[0])]
    res = {k: np.array([o[k] for o in out]) for k in ("K", "X", "resid", "iters", "status")}
    res["margin"] = np.array([o.get("margin", np.nan) for o in out])
    return res


def closed(Phi, Gam, Cm, D, K):
    """(Phi - Gam K, C - D K) of a batch the way the kernel sums them: from Phi (C), minus the columns of Gam (D) ascending"""
    Pc, Cc = Phi.copy(), Cm.copy()
    for a in range(Gam.shape[2]):
        Pc = Pc - Gam[:, :, a:a + 1] * K[:, a:a + 1, :]
        Cc = Cc - D[:, :, a:a + 1] * K[:, a:a + 1, :]
    return Pc, Cc


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------------
def scipy_dlqr(Phi, Gam, Q, R):
    """(K, X) of one system from scipy's solver of the discrete equation"""
    from scipy.linalg import solve_discrete_are
    X = solve_discrete_are(Phi, Gam, Q, R)
    return np.linalg.solve(R + Gam.T @ X @ Gam, Gam.T @ X @ Phi), X


def scipy_batch(Phi, Gam, Q, R):
    out = [scipy_dlqr(Phi[i], Gam[i], Q, R) for i in range(Phi.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def residual(Phi, Gam, Q, K, X):
    """the residual of fb_lss_dlqr's contract for any (K, X)"""
    E = Phi.T @ X @ Phi - X - Phi.T @ X @ Gam @ K + Q
    return float(np.abs(E).max() / max(np.abs(Q).max(), np.abs(X).max()))


def rho(M):
    return float(np.abs(np.linalg.eigvals(M)).max())


def designs(Phi, Gam, Q, R):
    """the prototype's and scipy's designs of one batch, computed once and read only: (dict of the prototype's, Ks, Xs)"""
    got = dlqr_batch(Phi, Gam, Q, R)
    Ks, Xs = scipy_batch(Phi, Gam, Q, R)
    for a in (Ks, Xs, *got.values()):
        a.setflags(write=False)
    return got, Ks, Xs


def sensitivity(Phi, Gam, K, terms=4096):
    """sum_k |Phic^k|_2^2 with Phic = Phi - Gam K: a bound on the 2-norm of the inverse of the closed loop's Stein operator dX -> dX - Phic' dX Phic,
    which carries a residual of the Riccati equation into the error of its solution (to first order)"""
    Pc = Phi - Gam @ K
    P, s = np.eye(Phi.shape[0]), 0.0
    for _ in range(terms):
        nrm = np.linalg.norm(P, 2)
        s += nrm * nrm
        if nrm < 1e-9:
            break
        P = P @ Pc
    return s


rel_dev = lq.rel_dev


def cost(Phi, Gam, Q, R, K, X, dx0, M):
    """(sum over M samples of dx' Q dx + u' R u with u = -K dx along c2d_prototype.map_steps, dx0' X dx0, |dx_M|_inf / |dx0|_inf) of one
    batch [n, ...] under the closed map Phi - Gam K"""
    n, nx = dx0.shape
    Pc = closed(Phi, Gam, np.zeros((n, 1, nx)), np.zeros((n, 1, Gam.shape[2])), K)[0]
    z, zu = np.zeros((n, nx)), np.zeros((n, 1))
    x, J = dx0.copy(), np.zeros(n)
    for _ in range(M):
        J = J + stage_cost(x, K, Q, R)
        x = c2d.map_steps(Pc, np.zeros((n, nx, 1)), z, z, zu, x, zu, 1)
    return J, np.einsum("ni,nij,nj->n", dx0, X, dx0), np.abs(x).max(axis=1) / np.abs(dx0).max(axis=1)


def stage_cost(dx, K, Q, R):
    u = -np.einsum("nij,nj->ni", K, dx)
    return np.einsum("ni,ij,nj->n", dx, Q, dx) + np.einsum("ni,ij,nj->n", u, R, u)
