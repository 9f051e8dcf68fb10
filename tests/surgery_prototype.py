"""The algorithms of fb_lss_transform and fb_lss_steady restated in numpy (test infrastructure; kernels: csrc/surgery_kernels.hpp;
docs/design/linearize.md, "Design-model surgery on the device"), in float64 and in np.longdouble (their own Gauss-Jordan elimination:
np.linalg does not take longdouble), and the generators of the random cases.

    solve       Gauss-Jordan elimination on [M | R] with the kernels' pivot rule: the pivot of step k is the not yet used row with the
                largest |M_ik| (ties: the lowest row), the rows stay where they are; the pivot row is scaled by the reciprocal of its pivot;
                the row that was the pivot of step k ends as row k of inv(M) R. rpiv = smallest pivot magnitude / largest.
    transform   T = C[rows, :], Ti = solve(T, I); C' = C Ti, W = A Ti, [A' | B' | xdot0'] = T [W | B | xdot0], D' = D, x0' = y0[rows]
    steady      L = [A B; C[iz, :] D[iz, :]], [X; U] = solve(L, [0; I]); K_fwd = U + K X

Every product is the kernels' sum: from 0 (from U for K_fwd), the terms added with k ascending. The kernels fuse each multiply-add; here
the product is rounded first: the two differ by rounding only, which the accuracy rule of tests/test_gpu_surgery.py allows for."""
import numpy as np

SINGULAR, NOT_FINITE, N_MAX = 1, 2, 32          # FB_SURGERY_SINGULAR, FB_SURGERY_NOT_FINITE, FB_SURGERY_N_MAX (include/flightbatch.h)
SEED = 61
N_SYS = 130
# (nx, nu, ny, nxo, nuo, nyo): every P of k_transform at its smallest and its largest size, ny > P; the last is the reference's full -> lon
T_SHAPES = ((1, 1, 1, 1, 1, 1), (8, 2, 9, 8, 2, 9), (9, 1, 17, 9, 1, 17), (16, 4, 33, 16, 4, 33), (17, 4, 20, 17, 4, 20), (32, 8, 64, 32, 8, 64),
            (20, 4, 38, 9, 2, 16))
# (nx, nz): every P of k_steady (P over nx + nz) at its smallest and its largest size
S_SHAPES = ((1, 1), (6, 2), (8, 8), (9, 2), (14, 2), (16, 8), (17, 1), (24, 8))


def group(rows):
    return 8 if rows <= 8 else 16 if rows <= 16 else 32


def mm(a, b, acc=None):
    """acc + a b with the terms added one k at a time, k ascending (acc None: from 0)"""
    out = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype) if acc is None else acc.copy()
    for k in range(a.shape[1]):
        out = out + np.outer(a[:, k], b[k])
    return out


def solve(M, R):
    """(inv(M) R, ok, rpiv) by Gauss-Jordan elimination, the kernels' way"""
    n = M.shape[0]
    W = np.concatenate([M, R], axis=1)
    used = np.zeros(n, dtype=bool)
    sigma = np.zeros(n, dtype=int)
    ok = True
    pmin, pmax = np.inf, 0.0
    with np.errstate(all="ignore"):
        for k in range(n):
            v = np.where(used, -1.0, np.abs(W[:, k]))
            m = np.nan if np.all(np.isnan(v)) else np.nanmax(v)
            cand = np.flatnonzero(~used & (v == m))
            if cand.size == 0 or not (m > 0.0) or not np.isfinite(m):
                ok = False
            if not np.isnan(m):
                pmin, pmax = min(pmin, float(m)), max(pmax, float(m))
            p = int(cand[0]) if cand.size else k
            ip = 1.0 / W[p, k]
            row = W[p] * ip
            f = W[:, k].copy()
            W = W - np.outer(f, row)
            W[p] = row
            used[p] = True
            sigma[k] = p
        rpiv = pmin / pmax if ok else 0.0
    return W[sigma, n:], ok, rpiv


def _verdict(ok, blocks):
    finite = all(np.all(np.isfinite(np.asarray(b, dtype=np.float64))) for b in blocks)
    return NOT_FINITE if not finite else (0 if ok else SINGULAR)


def transform(m, rows, zero=None, dtype=np.float64):
    """(A', B', C', D', xdot0', x0', status, rpiv) of one system m = (xdot0, x0, u0, y0, A, B, C, D); a flagged system has NaN matrices and xdot0'"""
    xdot0, x0, u0, y0, A, B, C, D = (np.asarray(b).astype(dtype) for b in m)
    rows = np.asarray(rows, dtype=int)
    nx = A.shape[0]
    T = C[rows]
    with np.errstate(all="ignore"):
        Ti, ok, rpiv = solve(T, np.eye(nx, dtype=dtype))
        Cp = mm(C, Ti)
        W = mm(A, Ti)
        out = mm(T, np.concatenate([W, B, xdot0[:, None]], axis=1))
    Ap, Bp, xd = out[:, :nx], out[:, nx:-1], out[:, -1].copy()
    if zero is not None:
        xd[np.asarray(zero, dtype=bool)] = 0.0
    status = _verdict(ok, (A, B, C, D, xdot0))
    res = [Ap, Bp, Cp, D.copy(), xd]
    if status:
        res = [np.full(b.shape, np.nan, dtype=dtype) for b in res]
        rpiv = np.nan if status == NOT_FINITE else 0.0
    return tuple(res) + (y0[rows], status, rpiv)


def steady(m, iz, K=None, dtype=np.float64):
    """(X, U, K_fwd or None, status, rpiv) of one system m = (A, B, C, D)"""
    A, B, C, D = (np.asarray(b).astype(dtype) for b in m)
    iz = np.asarray(iz, dtype=int)
    nx, nu = B.shape
    L = np.block([[A, B], [C[iz], D[iz]]])
    R = np.concatenate([np.zeros((nx, nu), dtype=dtype), np.eye(nu, dtype=dtype)])
    with np.errstate(all="ignore"):
        S, ok, rpiv = solve(L, R)
        X, U = S[:nx], S[nx:]
        Kf = None if K is None else mm(np.asarray(K).astype(dtype), X, U)
    status = _verdict(ok, (L,) if K is None else (L, K))
    if status:
        X, U = np.full(X.shape, np.nan, dtype=dtype), np.full(U.shape, np.nan, dtype=dtype)
        Kf = None if K is None else np.full(U.shape, np.nan, dtype=dtype)
        rpiv = np.nan if status == NOT_FINITE else 0.0
    return X, U, Kf, status, rpiv


def _batch(results, nmat):
    return tuple(np.array([r[k] for r in results]) for k in range(nmat))


def transform_batch(M, rows, zero=None, dtype=np.float64):
    """the same over a batch: M a tuple of [N, ...] arrays; returns (A', B', C', D', xdot0', x0', status [N], rpiv [N])"""
    n = M[0].shape[0]
    res = [transform(tuple(b[i] for b in M), rows, zero, dtype) for i in range(n)]
    return _batch(res, 6) + (np.array([r[6] for r in res], dtype=np.int32), np.array([r[7] for r in res], dtype=np.float64))


def steady_batch(M, iz, K=None, dtype=np.float64):
    """(X, U, K_fwd, status [N], rpiv [N]); K [nu, nx] for the batch, [N, nu, nx] per system or None"""
    n = M[0].shape[0]
    per = lambda i: None if K is None else (K[i] if np.ndim(K) == 3 else K)
    res = [steady(tuple(b[i] for b in M), iz, per(i), dtype) for i in range(n)]
    Kf = None if K is None else np.array([r[2] for r in res])
    return (np.array([r[0] for r in res]), np.array([r[1] for r in res]), Kf, np.array([r[3] for r in res], dtype=np.int32),
            np.array([r[4] for r in res], dtype=np.float64))


def subsystem(blocks, ix, iu, iy):
    """(A, B, C, D, xdot0, x0) [N, ...] through the selection lists"""
    A, B, C, D, xd, x0 = blocks
    return (A[:, ix][:, :, ix], B[:, ix][:, :, iu], C[:, iy][:, :, ix], D[:, iy][:, :, iu], xd[:, ix], x0[:, ix])


# ---- the random cases ---------------------------------------------------------------------------------------------------------------------------
def well_conditioned(rng, n, m):
    """n matrices Π (I + 0.5 G / sqrt(m)): Π a random row permutation, G standard normal"""
    out = np.eye(m) + 0.5 * rng.standard_normal((n, m, m)) / np.sqrt(m)
    for i in range(n):
        out[i] = out[i][rng.permutation(m)]
    return out


def t_case(shape, n=N_SYS, seed=SEED):
    """(M, rows, zero, ix, iu, iy): M = (xdot0, x0, u0, y0, A, B, C, D) of n random systems whose rows `rows` of C hold a well-conditioned T;
    a random xdot_zero mask (never the whole vector); selection lists that reorder, and drop where the shape's new sizes are smaller"""
    nx, nu, ny, nxo, nuo, nyo = shape
    rng = np.random.default_rng([seed, *shape])
    mk = lambda *s: rng.standard_normal(s)
    M = [mk(n, nx), mk(n, nx), mk(n, nu), mk(n, ny), mk(n, nx, nx) / np.sqrt(nx), mk(n, nx, nu), mk(n, ny, nx), mk(n, ny, nu)]
    rows = rng.permutation(ny)[:nx].astype(np.int32)
    M[6][:, rows] = well_conditioned(rng, n, nx)
    zero = (rng.random(nx) < 0.3).astype(np.int32)
    zero[0] = 0
    ix, iu, iy = (rng.permutation(a)[:b].astype(np.int32) for a, b in ((nx, nxo), (nu, nuo), (ny, nyo)))
    return tuple(M), rows, zero, ix, iu, iy


def s_case(shape, n=N_SYS, seed=SEED):
    """(M, iz, K, K_wide): M = (A, B, C, D) of n random systems with ny = nz + 3 outputs whose L = [A B; C[iz] D[iz]] is well conditioned;
    K [n, nu, nx] per system and K_wide [nu, nx] for the batch.
    A block of few entries can be small by cancellation however well L is conditioned (nz = 1: U and K_fwd are single numbers), and a
    deviation divided by it says nothing; a draw (L, K) is therefore taken only if max|U| >= 0.1 and max|U + K X| >= 0.1 max(|U| + |K| |X|), the size of the terms K_fwd is summed from, with K and with K_wide."""
    nx, nz = shape
    rng = np.random.default_rng([seed, 7, *shape])
    m, ny = nx + nz, nz + 3
    L, K, K_wide = np.empty((n, m, m)), np.empty((n, nz, nx)), rng.standard_normal((nz, nx))
    for i in range(n):
        while True:
            L[i], K[i] = well_conditioned(rng, 1, m)[0], rng.standard_normal((nz, nx))
            Mi = np.linalg.inv(L[i])
            U, X = Mi[nx:, nx:], Mi[:nx, nx:]
            if np.abs(U).max() >= 0.1 and all(np.abs(U + k @ X).max() >= 0.1 * (np.abs(U) + np.abs(k) @ np.abs(X)).max() for k in (K[i], K_wide)):
                break
    iz = rng.permutation(ny)[:nz].astype(np.int32)
    C, D = rng.standard_normal((n, ny, nx)), rng.standard_normal((n, ny, nz))
    C[:, iz], D[:, iz] = L[:, nx:, :nx], L[:, nx:, nx:]
    return (L[:, :nx, :nx].copy(), L[:, :nx, nx:].copy(), C, D), iz, K, K_wide


def block_dev(got, want):
    """the worst |got - want| over a block divided by the block's largest |want|, per system: [N]"""
    got, want = np.asarray(got), np.asarray(want)
    n = want.shape[0]
    d = np.abs(got.astype(np.longdouble) - want).reshape(n, -1).max(axis=1)
    return (d / np.abs(want).reshape(n, -1).max(axis=1)).astype(np.float64)


def dc_gain(m, iz, K, K_fwd):
    """the DC gain from r to z[iz] of one system under u = K_fwd r - K x, in longdouble: (C_z - D_z K) inv(-(A - B K)) B K_fwd + D_z K_fwd"""
    ld = np.longdouble
    A, B, C, D = (np.asarray(b).astype(ld) for b in m)
    K, Kf = np.asarray(K).astype(ld), np.asarray(K_fwd).astype(ld)
    iz = np.asarray(iz, dtype=int)
    x, ok, _ = solve(-(A - B @ K), B @ Kf)
    assert ok
    return (C[iz] - D[iz] @ K) @ x + D[iz] @ Kf


_SIDES = {}


def t_sides(shape):
    """(case, float64 result, longdouble result) of a transform shape over N_SYS systems, before the selection lists; computed once, shared"""
    key = ("t",) + tuple(shape)
    if key not in _SIDES:
        cs = t_case(shape)
        _SIDES[key] = (cs, transform_batch(cs[0], cs[1], cs[2], np.float64), transform_batch(cs[0], cs[1], cs[2], np.longdouble))
    return _SIDES[key]


def s_sides(shape, wide=False):
    """(case, float64 result, longdouble result) of a steady-map shape over N_SYS systems, with K per system or K_wide for the batch"""
    key = ("s", wide) + tuple(shape)
    if key not in _SIDES:
        cs = s_case(shape)
        K = cs[3] if wide else cs[2]
        _SIDES[key] = (cs, steady_batch(cs[0], cs[1], K, np.float64), steady_batch(cs[0], cs[1], K, np.longdouble))
    return _SIDES[key]
