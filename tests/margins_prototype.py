"""The algorithm of fb_lss_margins restated in numpy fp64, one system at a time (test infrastructure; kernel: csrc/margins_kernels.hpp;
contract: include/flightbatch.h; docs/design/linearize.md, "Margins on the device"): the same brackets on the grid, the same geometric
bisection, the same selection, L(jω) by a complex Gauss-Jordan elimination with the family's pivot rule on |z|². Beside it the exact side
(numpy.linalg.solve for L, scipy.optimize.brentq inside the same grid brackets), the deviation measure of the family's rule, and the
generators of tests/test_margins_host.py and tests/test_gpu_margins.py.

A system is (A [nx, nx], b [nx], c [nx], d): the channel the loop is closed around. A result is (sel [10], counts [2], all [6, KMAX],
status), laid out as fb_lss_margins lays out one system."""
import functools

import numpy as np

NOT_FINITE, SINGULAR, TRUNCATED, KMAX, NX_MAX, ITERS = 1, 2, 4, 8, 32, 60
FLOOR, FACTOR = 1e-11, 10.0        # the family's rule: the device may deviate FACTOR times as far as the prototype, at least FLOOR
FAIR_GRID, FAIR_GM, PROTO_MAX = 1e-9, 1e-3, 1e-9
NX_CLOSED = (3, 7, 8, 9, 16, 17, 31, 32)
K_CLOSED = (2.0, 4.0, 7.0)
W_CLOSED = np.logspace(-2.0, 2.0, 33)
N_BIG = 130


# ---- L(jω) ---------------------------------------------------------------------------------------------------------------------------------
def response(A, b, c, d, om):
    """(c inv(jωI - A) b + d, ok): Gauss-Jordan on the rows of [jωI - A | b], the pivot of step k the largest |z|² among the rows not yet
    used, the lowest row at a tie; not ok when that is zero or not finite, or the value is not finite"""
    nx = A.shape[0]
    Z = np.empty((nx, nx + 1), dtype=np.complex128)
    Z[:, :nx] = 1j * om * np.eye(nx) - A
    Z[:, nx] = b
    used, who = np.zeros(nx, dtype=bool), np.empty(nx, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(nx):
            m2 = Z[:, k].real ** 2 + Z[:, k].imag ** 2
            m2[used] = -1.0
            p = int(np.argmax(m2))
            if not (m2[p] > 0.0 and np.isfinite(m2[p])):
                return complex(np.nan, np.nan), False
            Z[p, k + 1:] *= np.conj(Z[p, k]) / m2[p]
            f = Z[:, k].copy()
            f[p] = 0.0
            Z[:, k + 1:] -= np.outer(f, Z[p, k + 1:])
            used[p], who[k] = True, p
        v = d + np.dot(c, Z[who, nx])
    return v, bool(np.isfinite(v.real) and np.isfinite(v.imag))


def exact_response(A, b, c, d, om):
    return d + np.dot(c, np.linalg.solve(1j * om * np.eye(A.shape[0]) - A, b.astype(np.complex128)))


# ---- the contract --------------------------------------------------------------------------------------------------------------------------
def _before(kind, L):
    return L.imag < 0.0 if kind == 0 else L.real * L.real + L.imag * L.imag < 1.0


def brackets(L):
    """the indices of the intervals that bracket a phase crossing, a gain crossing"""
    im_neg, inside = L.imag < 0.0, L.real ** 2 + L.imag ** 2 < 1.0
    ph = (im_neg[:-1] != im_neg[1:]) & ~((L.real[:-1] >= 0.0) & (L.real[1:] >= 0.0))
    return np.flatnonzero(ph), np.flatnonzero(inside[:-1] != inside[1:])


def closer_to_one(g, h):
    """max(g, 1 / g) < max(h, 1 / h) without dividing"""
    if g >= 1.0 and h >= 1.0:
        return g < h
    if g < 1.0 and h < 1.0:
        return g > h
    return g * h < 1.0 if g >= 1.0 else g * h > 1.0


def _void(status):
    return np.full(10, np.nan), np.zeros(2, dtype=np.int32), np.full((6, KMAX), np.nan), status


def _finish(L, w, found, trunc):
    """sel, counts, all and the status from the kept crossings found[kind] = [(ω*, L*), ...] in ascending frequency"""
    sel, allv = np.full(10, np.nan), np.full((6, KMAX), np.nan)
    for kind in (0, 1):
        for s, (om, v) in enumerate(found[kind]):
            allv[3 * kind:3 * kind + 3, s] = om, v.real, v.imag
    sel[0] = sel[2] = np.inf
    if found[0]:
        best = 0
        for s in range(1, len(found[0])):
            if closer_to_one(-found[0][s][1].real, -found[0][best][1].real):
                best = s
        om, v = found[0][best]
        sel[0], sel[1], sel[4], sel[5] = -1.0 / v.real, om, v.real, v.imag
    if found[1]:
        key = lambda v: (-v.real * abs(v.real), v.real * v.real + v.imag * v.imag)
        best = 0
        for s in range(1, len(found[1])):
            (n1, d1), (n0, d0) = key(found[1][s][1]), key(found[1][best][1])
            if n1 * d0 > n0 * d1:
                best = s
        om, v = found[1][best]
        sel[2], sel[3], sel[6], sel[7] = np.degrees(np.arctan2(-v.imag, -v.real)), om, v.real, v.imag
    s2 = (1.0 + L.real) ** 2 + L.imag ** 2
    k = int(np.argmin(s2))
    sel[8], sel[9] = np.sqrt(s2[k]), w[k]
    return sel, np.array([len(found[0]), len(found[1])], dtype=np.int32), allv, TRUNCATED if trunc else 0


def margins(A, b, c, d, w, gain=1.0):
    """fb_lss_margins of one system"""
    if not (np.isfinite(A).all() and np.isfinite(b).all() and np.isfinite(c).all() and np.isfinite(d) and np.isfinite(gain)):
        return _void(NOT_FINITE)
    L = np.empty(w.size, dtype=np.complex128)
    for k, om in enumerate(w):
        v, ok = response(A, b, c, d, om)
        v = complex(gain * v.real, gain * v.imag)
        if not (ok and np.isfinite(v.real) and np.isfinite(v.imag)):
            return _void(SINGULAR)
        L[k] = v
    found, trunc = ([], []), False
    for kind, ks in enumerate(brackets(L)):
        for k in ks:
            if kind == 1 and len(found[1]) == KMAX:     # a gain bracket always counts: nothing to refine
                trunc = True
                break
            lo, hi, llo = w[k], w[k + 1], L[k]
            plo = _before(kind, llo)
            for _ in range(ITERS):
                mid = np.sqrt(lo * hi)
                if not lo < mid < hi:
                    break
                v, ok = response(A, b, c, d, mid)
                if not ok:
                    return _void(SINGULAR)
                v = complex(gain * v.real, gain * v.imag)
                if _before(kind, v) == plo:
                    lo, llo = mid, v
                else:
                    hi = mid
            if kind == 0 and not llo.real < 0.0:
                continue
            if len(found[kind]) == KMAX:
                trunc = True
                break
            found[kind].append((lo, llo))
    return _finish(L, w, found, trunc)


def exact(A, b, c, d, w, gain=1.0):
    """the exact side: LAPACK for L, Brent's root finder inside the same grid brackets, the same acceptance and selection"""
    from scipy.optimize import brentq
    f = lambda om: gain * exact_response(A, b, c, d, om)
    L = np.array([f(om) for om in w])
    g = (lambda om: f(om).imag, lambda om: abs(f(om)) ** 2 - 1.0)
    found, trunc = ([], []), False
    for kind, ks in enumerate(brackets(L)):
        for k in ks:
            if len(found[kind]) == KMAX and kind == 1:
                trunc = True
                break
            om = brentq(g[kind], w[k], w[k + 1], xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)
            v = f(om)
            if kind == 0 and not v.real < 0.0:
                continue
            if len(found[kind]) == KMAX:
                trunc = True
                break
            found[kind].append((om, v))
    return _finish(L, w, found, trunc), L


def deviation(got, ex):
    """the worst of: ω* relative, gm relative, pm in degrees / 180, over the selected and every kept crossing; smin relative. The counts
    and the status must be equal."""
    (sel, counts, allv, status), (sel_e, counts_e, all_e, status_e) = got, ex
    assert status == status_e and tuple(counts) == tuple(counts_e), (status, status_e, counts, counts_e)
    rel = lambda x, y: abs(x - y) / abs(y)
    dev = [rel(sel[8], sel_e[8])]
    assert sel[9] == sel_e[9]
    for kind in (0, 1):
        for s in range(counts[kind]):
            om, v, om_e, v_e = allv[3 * kind, s], complex(*allv[3 * kind + 1:3 * kind + 3, s]), all_e[3 * kind, s], complex(*all_e[3 * kind + 1:3 * kind + 3, s])
            dev.append(rel(om, om_e))
            dev.append(rel(-1.0 / v.real, -1.0 / v_e.real) if kind == 0 else abs(np.degrees(np.arctan2(-v.imag, -v.real) - np.arctan2(-v_e.imag, -v_e.real))) / 180.0)
    if counts[0]:
        dev += [rel(sel[1], sel_e[1]), rel(sel[0], sel_e[0])]
    else:
        assert sel[0] == sel_e[0] == np.inf and np.isnan(sel[1])
    if counts[1]:
        dev += [rel(sel[3], sel_e[3]), abs(sel[2] - sel_e[2]) / 180.0]
    else:
        assert sel[2] == sel_e[2] == np.inf and np.isnan(sel[3])
    return float(max(dev))


def fairness(L, ex):
    """(min |Im L_k| / |L_k|, min | |L_k|² - 1 |, min accepted -Re L*) of the exact side"""
    m = np.abs(L)
    allv, counts = ex[2], ex[1]
    return float((np.abs(L.imag) / m).min()), float(np.abs(m * m - 1.0).min()), float(min([-allv[1, s] for s in range(counts[0])], default=np.inf))


def from_device(sel, counts, allv, status, i):
    """system i of fb_lss_margins' arrays ([10, N], [2, N], [6, KMAX, N] or None, [N]) as a result"""
    return sel[:, i].copy(), counts[:, i].copy(), (np.full((6, KMAX), np.nan) if allv is None else allv[:, :, i].copy()), int(status[i])


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def tf(num, den):
    """(A, b, c, d) of num(s) / den(s), coefficients in descending powers, in controllable companion form (strictly proper or proper)"""
    den = np.asarray(den, dtype=np.float64)
    num = np.concatenate([np.zeros(den.size - len(num)), np.asarray(num, dtype=np.float64)]) / den[0]
    den = den / den[0]
    nx = den.size - 1
    A = np.zeros((nx, nx))
    A[0] = -den[1:]
    A[1:, :-1] = np.eye(nx - 1)
    b = np.zeros(nx); b[0] = 1.0
    d = num[0]
    return A, b, num[1:] - d * den[1:], d


def embed(sys, nx, rng, rotate=True):
    """the system among nx states: the extra ones stable, driven by the input and the plant, unobservable; then a random orthogonal change
    of state (the Q of a QR factorisation)"""
    A0, b0, c0, d = sys
    n0 = A0.shape[0]
    A, b, c = np.zeros((nx, nx)), np.zeros(nx), np.zeros(nx)
    A[:n0, :n0], b[:n0], c[:n0] = A0, b0, c0
    if nx > n0:
        F = rng.standard_normal((nx - n0, nx - n0))
        F -= (np.linalg.eigvals(F).real.max() + 0.5) * np.eye(nx - n0)
        A[n0:, n0:], A[n0:, :n0], b[n0:] = F, rng.standard_normal((nx - n0, n0)), rng.standard_normal(nx - n0)
    if rotate and nx > 1:
        Q = np.linalg.qr(rng.standard_normal((nx, nx)))[0]
        A, b, c = Q @ A @ Q.T, Q @ b, c @ Q.T
    return A, b, c, d


def cube(K):
    """K / (s + 1)³ as a chain"""
    return np.array([[-1.0, 1.0, 0.0], [0.0, -1.0, 1.0], [0.0, 0.0, -1.0]]), np.array([0.0, 0.0, 1.0]), np.array([K, 0.0, 0.0]), 0.0


def cube_closed_form(K):
    """gm, wpc, pm (degrees), wgc of K / (s + 1)³"""
    wgc = np.sqrt(K ** (2.0 / 3.0) - 1.0)
    return 8.0 / K, np.sqrt(3.0), 180.0 - 3.0 * np.degrees(np.arctan(wgc)), wgc


VARIANTS = 4      # distinct changes of state per K: a batch cycles through len(K_CLOSED) * VARIANTS systems, 12 never divides its sizes


@functools.lru_cache(maxsize=None)
def closed_systems(nx):
    """the distinct systems of the closed-form batches at this nx, with K of each"""
    rng = np.random.default_rng(1000 + nx)
    return [(embed(cube(K), nx, rng), K) for _ in range(VARIANTS) for K in K_CLOSED]


def conditionally_stable():
    """2 (s + 1)² / (s³ (s / 20 + 1)²): two phase crossings, the selected gain margin below 1; one gain crossing"""
    return tf(2.0 * np.array([1.0, 2.0, 1.0]), np.polymul([1.0, 0.0, 0.0, 0.0], np.polymul([0.05, 1.0], [0.05, 1.0])))


def modes(m=6, zeta=0.05, a=0.3, w0=0.5, ratio=2.0):
    """the sum of m lightly damped modes a ω² / (s² + 2 ζ ω s + ω²): two gain crossings a mode, no phase crossing (Im L < 0 throughout)"""
    A, b, c = np.zeros((2 * m, 2 * m)), np.zeros(2 * m), np.zeros(2 * m)
    for k in range(m):
        om = w0 * ratio ** k
        A[2 * k:2 * k + 2, 2 * k:2 * k + 2] = [[0.0, 1.0], [-om * om, -2.0 * zeta * om]]
        b[2 * k + 1], c[2 * k] = 1.0, a * om * om
    return A, b, c, 0.0


W_MODES = np.logspace(-1.0, 2.5, 257)
W_WORK = np.logspace(-2.0, 3.0, 161)
NX_WORK = 6


def work_kinds():
    """name -> system: 0, 1, 2 and 3 crossings, for the batch whose neighbours do unequal work (all of at most NX_WORK states)"""
    return {"none": tf([0.5], [1.0, 1.0]), "one": tf([3.0], [1.0, 1.0, 0.0]), "two": cube(4.0), "three": conditionally_stable(),
            "first-order": tf([3.0], [1.0, 1.0])}


@functools.lru_cache(maxsize=None)
def work_systems():
    """the N_BIG systems of the unequal-work batch: the kinds in turn, every system with its own extra states and change of state"""
    rng = np.random.default_rng(77)
    kinds = work_kinds()
    names = list(kinds)
    return [(names[i % len(names)], embed(kinds[names[i % len(names)]], NX_WORK, rng)) for i in range(N_BIG)]


def edge_grid(K, nw):
    """a grid whose first interval holds the gain crossing of K / (s + 1)³ and whose last interval holds its phase crossing"""
    gm, wpc, pm, wgc = cube_closed_form(K)
    r = (wpc / wgc) ** (1.0 / (nw - 2))           # each crossing at the geometric middle of its interval
    return wgc * r ** (np.arange(nw) - 0.5)


def lss_arrays(systems, nu=2, ny=2, iu=1, iy=1, seed=5):
    """dict(A, B, C, D, xdot0, x0, u0, y0) [n, ...] with every system's channel at (iu, iy), the other entries random"""
    rng = np.random.default_rng(seed)
    n, nx = len(systems), systems[0][0].shape[0]
    M = dict(A=np.array([s[0] for s in systems]), B=rng.standard_normal((n, nx, nu)), C=rng.standard_normal((n, ny, nx)),
             D=rng.standard_normal((n, ny, nu)), xdot0=rng.standard_normal((n, nx)), x0=rng.standard_normal((n, nx)),
             u0=rng.standard_normal((n, nu)), y0=rng.standard_normal((n, ny)))
    for i, s in enumerate(systems):
        M["B"][i, :, iu], M["C"][i, iy, :], M["D"][i, iy, iu] = s[1], s[2], s[3]
    return M
