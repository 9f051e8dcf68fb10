"""The algorithm of fb_lss_connect restated in numpy (test infrastructure; kernel: csrc/connect_kernels.hpp; docs/design/linearize.md,
"Closing loops on the device"), in float64 and in np.longdouble (the family's Gauss-Jordan elimination, surgery_prototype.solve: np.linalg
does not take longdouble), and the generator of the random cases.

    stacked   v = [u_p; u_c], z = [y_p; y_c], x = [x_p; x_c]; A, B, C, D block-diagonal
    rows      W = [I - F D[jz, :] | F C[jz, :] | G], one row per entry of v
    E         [M | Nw] = solve(I - F D[jz, :], [F C[jz, :] | G]), the one numpy statement of the device's solve (fbg::gj_solve)
    result    A' = A + B M, B' = B Nw, C' = C[iz, :] + D[iz, :] M, D' = D[iz, :] Nw

The sums over k run with k ascending, as in the kernel; the products are numpy's matmul (each sum formed first, then added), where the
kernel starts from the term it adds to and fuses every multiply-add: the two differ by rounding only, which the accuracy rule of
tests/test_gpu_connect.py allows for. Where F D[jz, :] = 0 every pivot is exactly 1 and M = F C[jz, :], Nw = G to the last bit."""
import numpy as np

from surgery_prototype import block_dev, solve  # noqa: F401  (block_dev: the tests reach it through this module)

ILL_POSED, NOT_FINITE = 1, 2          # FB_CONNECT_ILL_POSED, FB_CONNECT_NOT_FINITE (include/flightbatch.h)
NV_MAX, NF_MAX, NZ_MAX = 16, 32, 128
SEED = 59
N_SYS = 130
# (nx_p, nx_c, nu_p, nu_c, ny_p, ny_c, nf, nw, ny); nx_c = 0: no compensator. Every P of the kernel at its smallest and its largest size; the
# tenth and eleventh give the compensator the handle group sizes 8 and 32 (the plant has 4, 8, 16 and 32 among the first nine, the compensator
# 4 and 16), the last is P = 32 at its smallest size, 17 states.
SHAPES = ((1, 0, 1, 0, 1, 0, 1, 1, 1), (4, 1, 1, 1, 6, 1, 4, 1, 7), (7, 1, 2, 1, 3, 1, 2, 2, 4), (8, 1, 2, 1, 8, 1, 9, 1, 1),
          (15, 1, 4, 1, 33, 1, 16, 4, 34), (16, 16, 8, 8, 64, 64, 32, 8, 64), (20, 2, 4, 1, 38, 1, 5, 2, 39), (28, 4, 8, 8, 64, 8, 32, 8, 64),
          (31, 1, 7, 1, 63, 1, 32, 8, 64), (4, 7, 1, 1, 3, 2, 3, 2, 4), (3, 20, 1, 2, 2, 3, 3, 2, 4), (16, 1, 2, 1, 3, 1, 2, 2, 4))


def group(nx, nv):
    m = max(nx, nv)
    return 8 if m <= 8 else 16 if m <= 16 else 32


def handle_group(nx):
    return 4 if nx <= 4 else 8 if nx <= 8 else 16 if nx <= 16 else 32


def stack(p, c, dtype=np.float64):
    """the block-diagonal (A, B, C, D) of plant p and compensator c (None: the plant alone), each a tuple (A, B, C, D) of one system"""
    p = tuple(np.asarray(m).astype(dtype) for m in p)
    if c is None:
        return p
    c = tuple(np.asarray(m).astype(dtype) for m in c)
    out = []
    for mp, mc in zip(p, c):
        m = np.zeros((mp.shape[0] + mc.shape[0], mp.shape[1] + mc.shape[1]), dtype=dtype)
        m[:mp.shape[0], :mp.shape[1]] = mp
        m[mp.shape[0]:, mp.shape[1]:] = mc
        out.append(m)
    return tuple(out)


def connect(p, c, jz, F, G, iz, dtype=np.float64):
    """(A', B', C', D', status) of one system; a system with a non-zero status has NaN matrices"""
    A, B, C, D = stack(p, c, dtype)
    F, G = np.asarray(F).astype(dtype), np.asarray(G).astype(dtype)
    jz = np.asarray(jz, dtype=int)
    iz = np.arange(C.shape[0]) if iz is None else np.asarray(iz, dtype=int)
    nx, nv = B.shape
    nw = G.shape[1]
    with np.errstate(all="ignore"):
        S, ok, _ = solve(np.eye(nv, dtype=dtype) - F @ D[jz], np.concatenate([F @ C[jz], G], axis=1))
        M, Nw = S[:, :nx], S[:, nx:]
        out = (A + B @ M, B @ Nw, C[iz] + D[iz] @ M, D[iz] @ Nw)
    finite = all(np.all(np.isfinite(m)) for m in (A, B, C, D, F, G))
    status = NOT_FINITE if not finite else (0 if ok else ILL_POSED)
    if status:
        out = tuple(np.full(m.shape, np.nan, dtype=dtype) for m in out)
    return out + (status,)


def connect_batch(P, Cc, jz, F, G, iz, dtype=np.float64):
    """the same over a batch: P, Cc tuples of [N, ., .] arrays (Cc None: no compensator), F, G [., .] for the batch or [N, ., .] per system"""
    n = P[0].shape[0]
    per = lambda M, i: M[i] if np.ndim(M) == 3 else M
    res = [connect(tuple(m[i] for m in P), None if Cc is None else tuple(m[i] for m in Cc), jz, per(F, i), per(G, i), iz, dtype) for i in range(n)]
    return tuple(np.array([r[k] for r in res]) for k in range(4)) + (np.array([r[4] for r in res], dtype=np.int32),)


# ---- the random cases ---------------------------------------------------------------------------------------------------------------------------
def case(shape, n=N_SYS, seed=SEED):
    """plant and compensator (tuples of [n, ., .], the compensator None when nx_c = 0), jz, F [n, nv, nf], G [n, nv, nw], iz.
    A blocks are randn / sqrt(nx); B, C, D and G are randn; F is randn scaled so that ||F D[jz, :]||_2 = 0.5, hence cond(E) <= 3; jz and iz
    are random distinct rows of z in shuffled order."""
    nxp, nxc, nup, nuc, nyp, nyc, nf, nw, ny = shape
    rng = np.random.default_rng([seed, *shape])
    mk = lambda *s: rng.standard_normal(s)
    side = lambda nx, nu, ny_: (mk(n, nx, nx) / np.sqrt(nx), mk(n, nx, nu), mk(n, ny_, nx), mk(n, ny_, nu))
    P = side(nxp, nup, nyp)
    Cc = side(nxc, nuc, nyc) if nxc else None
    nv, nz = nup + nuc, nyp + nyc
    jz = rng.permutation(nz)[:nf].astype(np.int32)
    iz = rng.permutation(nz)[:ny].astype(np.int32)
    F = mk(n, nv, nf)
    for i in range(n):
        D = stack(tuple(m[i] for m in P), None if Cc is None else tuple(m[i] for m in Cc))[3]
        F[i] *= 0.5 / np.linalg.norm(F[i] @ D[jz], 2)
    return P, Cc, jz, F, mk(n, nv, nw), iz


_SIDES = {}


def sides(shape):
    """(case, float64 result, longdouble result) of a shape over N_SYS systems, computed once and shared (never modified)"""
    if shape not in _SIDES:
        cs = case(shape)
        _SIDES[shape] = (cs, connect_batch(*cs, dtype=np.float64), connect_batch(*cs, dtype=np.longdouble))
    return _SIDES[shape]


# ---- the compensators of flightbatch.connect, restated ------------------------------------------------------------------------------------------
def integrator():
    return np.zeros((1, 1)), np.ones((1, 1)), np.ones((1, 1)), np.zeros((1, 1))


def pid(p):
    """A = diag(0, -1 / tau_f), B = (1, 1 / tau_f)', C = (k_i, -k_d / tau_f), D = k_p + k_d / tau_f"""
    kp, ki, kd, tf = p
    return (np.array([[0.0, 0.0], [0.0, -1.0 / tf]]), np.array([[1.0], [1.0 / tf]]), np.array([[ki, -(kd / tf)]]), np.array([[kp + kd / tf]]))


def unity_feedback(p, c, iu=0, iy=0, dtype=np.float64):
    """flightbatch.connect.unity_feedback on one system: e = r - y[iy] into c, its output into plant input iu; outputs [y_p; y_c]"""
    nu, ny = p[1].shape[1], p[2].shape[0]
    F = np.zeros((nu + 1, 2)); F[iu, 1] = 1.0; F[nu, 0] = -1.0
    G = np.zeros((nu + 1, 1)); G[nu, 0] = 1.0
    return connect(p, c, [iy, ny], F, G, None, dtype)
