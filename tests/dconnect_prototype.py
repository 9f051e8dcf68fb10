"""The algorithm of fb_lss_dconnect restated in numpy (test infrastructure; kernel: csrc/dconnect_kernels.hpp; docs/design/linearize.md,
"Closing sampled loops on the device"), in float64 and in np.longdouble, the generator of the random cases, and a tick-by-tick reference.

    extend    xe = [x_p; x_c; q], ze = [y_p; y_c; q], q_k(t) = z[dz_k](t - 1):
              Ae = [[A, 0], [C[dz], 0]], Be = [B; D[dz]], Ce = [[C, 0], [0, I]], De = [D; 0]   (A, B, C, D: connect_prototype.stack)
    dconnect  connect_prototype.connect on the extended model: jz and iz index ze
    simulate  the interconnection itself, one tick at a time: the delay rows are a buffer that is written after the tick, the algebraic loop
              over the CURRENT reads is solved per tick by np.linalg.solve. It builds no extended matrix and does not use the formula.

The sums differ from the kernel's as connect_prototype's do (matmul against fused multiply-adds from the term they add to): rounding only,
which the accuracy rule of tests/test_gpu_dconnect.py allows for. Where no current read meets a feedthrough, every pivot is exactly 1."""
import numpy as np

import connect_prototype as cp
from connect_prototype import ILL_POSED, NOT_FINITE, group, handle_group, stack  # noqa: F401  (the tests reach them through this module)

ND_MAX = 31                           # FB_DCONNECT_ND_MAX (include/flightbatch.h)
SEED = 61
N_SYS = 130
TICKS = 12
# (nx_p, nx_c, nu_p, nu_c, ny_p, ny_c, nd, nf, nw, ny); nx_c = 0: no compensator. nx' = nx_p + nx_c + nd is 2, 8 | 9, 16 | 17, 32, 32, 28: both edges
# of every group size; the last has nd = 0 (nx' = 16)
SHAPES = ((1, 0, 1, 0, 1, 0, 1, 1, 1, 2), (4, 1, 1, 1, 6, 1, 3, 4, 1, 7), (5, 1, 2, 1, 3, 1, 3, 2, 2, 4), (8, 1, 2, 1, 8, 1, 7, 9, 1, 1),
          (9, 1, 4, 1, 20, 1, 7, 16, 4, 21), (16, 8, 8, 8, 40, 24, 8, 32, 8, 64), (20, 2, 4, 1, 38, 1, 10, 5, 2, 39), (3, 20, 1, 2, 2, 3, 5, 3, 2, 4),
          (15, 1, 4, 1, 33, 1, 0, 16, 4, 34))
ident = lambda s: "/".join(map(str, s))


def nxe(shape):
    return shape[0] + shape[1] + shape[6]


def block_dev(got, want):
    """surgery_prototype.block_dev, with a block whose largest |want| is 0 (D' of delayed outputs only) held to equality: 0 or inf"""
    got, want = np.asarray(got), np.asarray(want)
    n = want.shape[0]
    d = np.abs(got.astype(np.longdouble) - want).reshape(n, -1).max(axis=1).astype(np.float64)
    s = np.abs(want).reshape(n, -1).max(axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))


def extend(p, c, dz, dtype=np.float64):
    """(Ae, Be, Ce, De) of one system: the stacked model with the delay rows dz of z appended as states and as signals"""
    A, B, C, D = stack(p, c, dtype)
    dz = np.asarray(dz, dtype=int).reshape(-1)
    nx, nv = B.shape
    nz, nd = C.shape[0], dz.size
    Ae = np.zeros((nx + nd, nx + nd), dtype=dtype); Ae[:nx, :nx] = A; Ae[nx:, :nx] = C[dz]
    Be = np.concatenate([B, D[dz]], axis=0)
    Ce = np.zeros((nz + nd, nx + nd), dtype=dtype); Ce[:nz, :nx] = C; Ce[nz:, nx:] = np.eye(nd, dtype=dtype)
    De = np.concatenate([D, np.zeros((nd, nv), dtype=dtype)], axis=0)
    return Ae, Be, Ce, De


def dconnect(p, c, dz, jz, F, G, iz, dtype=np.float64):
    """(Phi', Gamma', C', D', status) of one system; a system with a non-zero status has NaN matrices"""
    return cp.connect(extend(p, c, dz, dtype), None, jz, F, G, iz, dtype)


def dconnect_batch(P, Cc, dz, jz, F, G, iz, dtype=np.float64):
    """the same over a batch: P, Cc tuples of [N, ., .] arrays (Cc None: no compensator), F, G [., .] for the batch or [N, ., .] per system"""
    n = P[0].shape[0]
    per = lambda M, i: M[i] if np.ndim(M) == 3 else M
    res = [dconnect(tuple(m[i] for m in P), None if Cc is None else tuple(m[i] for m in Cc), dz, jz, per(F, i), per(G, i), iz, dtype) for i in range(n)]
    return tuple(np.array([r[k] for r in res]) for k in range(4)) + (np.array([r[4] for r in res], dtype=np.int32),)


# ---- the interconnection, tick by tick -----------------------------------------------------------------------------------------------------------
def simulate(p, c, dz, jz, F, G, iz, w):
    """outputs [T, ny] of one system from rest under the inputs w [T, nw]: explicit delay buffers, the algebraic loop solved per tick"""
    A, B, C, D = stack(p, c)
    dz, jz = np.asarray(dz, dtype=int).reshape(-1), np.asarray(jz, dtype=int)
    nz, nv = D.shape
    iz = np.arange(nz + dz.size) if iz is None else np.asarray(iz, dtype=int)
    now, late = jz < nz, jz >= nz
    Fn, Fl = F[:, now], F[:, late]
    jn, jl = jz[now], jz[late] - nz
    x, q = np.zeros(A.shape[0]), np.zeros(dz.size)
    out = np.empty((w.shape[0], iz.size))
    for t in range(w.shape[0]):
        v = np.linalg.solve(np.eye(nv) - Fn @ D[jn], Fn @ (C[jn] @ x) + Fl @ q[jl] + G @ w[t])
        z = C @ x + D @ v
        out[t] = np.concatenate([z, q])[iz]
        x, q = A @ x + B @ v, z[dz]
    return out


def run(model, w):
    """outputs [T, ny] of x+ = Phi x + Gamma w, y = C x + D w from rest"""
    Phi, Gam, Cm, D = model
    x = np.zeros(Phi.shape[0])
    out = np.empty((w.shape[0], Cm.shape[0]))
    for t in range(w.shape[0]):
        out[t] = Cm @ x + D @ w[t]
        x = Phi @ x + Gam @ w[t]
    return out


def inputs(shape, n=N_SYS, ticks=TICKS, seed=SEED):
    """the random inputs [n, ticks, nw] of a shape's systems"""
    return np.random.default_rng([seed, 7, *shape]).standard_normal((n, ticks, shape[8]))


def run_dev(got, want):
    """max |got - want| over the ticks and outputs divided by the largest |want|, per system: [N]"""
    n = want.shape[0]
    return np.abs(got - want).reshape(n, -1).max(axis=1) / np.abs(want).reshape(n, -1).max(axis=1)


# ---- the random cases ---------------------------------------------------------------------------------------------------------------------------
def case(shape, n=N_SYS, seed=SEED):
    """plant and compensator (tuples of [n, ., .], the compensator None when nx_c = 0), dz, jz, F [n, nv, nf], G [n, nv, nw], iz: connect_prototype.case's
    generator. dz: random rows of z (a row may come twice); jz and iz: random distinct rows of [z; q] in shuffled order, jz redrawn until it
    holds a delayed row (nd > 0) and, where nf >= 2, a current one. F is randn scaled so that ||F De[jz, :]||_2 = 0.5 over the current reads,
    hence cond(E) <= 3; where no current read meets a feedthrough, ||F||_2 = 0.5."""
    nxp, nxc, nup, nuc, nyp, nyc, nd, nf, nw, ny = shape
    rng = np.random.default_rng([seed, *shape])
    mk = lambda *s: rng.standard_normal(s)
    side = lambda nx, nu, ny_: (mk(n, nx, nx) / np.sqrt(nx), mk(n, nx, nu), mk(n, ny_, nx), mk(n, ny_, nu))
    P = side(nxp, nup, nyp)
    Cc = side(nxc, nuc, nyc) if nxc else None
    nv, nz = nup + nuc, nyp + nyc
    dz = rng.integers(0, nz, size=nd).astype(np.int32)
    while True:
        jz = rng.permutation(nz + nd)[:nf].astype(np.int32)
        if (nd == 0 or (jz >= nz).any()) and (nd == 0 or nf < 2 or (jz < nz).any()):
            break
    iz = rng.permutation(nz + nd)[:ny].astype(np.int32)
    F = mk(n, nv, nf)
    for i in range(n):
        De = extend(tuple(m[i] for m in P), None if Cc is None else tuple(m[i] for m in Cc), dz)[3]
        s = np.linalg.norm(F[i] @ De[jz], 2)
        F[i] *= 0.5 / (s if s > 0 else np.linalg.norm(F[i], 2))
    return P, Cc, dz, jz, F, mk(n, nv, nw), iz


_SIDES = {}


def sides(shape):
    """(case, float64 result, longdouble result) of a shape over N_SYS systems, computed once and shared (never modified)"""
    if shape not in _SIDES:
        cs = case(shape)
        _SIDES[shape] = (cs, dconnect_batch(*cs, dtype=np.float64), dconnect_batch(*cs, dtype=np.longdouble))
    return _SIDES[shape]


_TICKS = {}


def tick_sides(shape):
    """(w [N, T, nw], the tick-by-tick reference [N, T, ny], the float64 result run over the same inputs [N, T, ny]) of a shape, shared"""
    if shape not in _TICKS:
        cs, f64, _ = sides(shape)
        P, Cc, dz, jz, F, G, iz = cs
        w = inputs(shape)
        take = lambda S, i: None if S is None else tuple(m[i] for m in S)
        ref = np.array([simulate(take(P, i), take(Cc, i), dz, jz, F[i], G[i], iz, w[i]) for i in range(w.shape[0])])
        got = np.array([run(tuple(m[i] for m in f64[:4]), w[i]) for i in range(w.shape[0])])
        _TICKS[shape] = (w, ref, got)
    return _TICKS[shape]
