"""The algorithms of fb_lss_dfreqresp and fb_lss_dmargins restated in numpy fp64, one system at a time (test infrastructure; kernels:
csrc/dfreq_kernels.hpp; contract: include/flightbatch.h; docs/design/linearize.md, "Sampled loops on the device"): the host's cos and sin
of θ_k = ω_k Ts, L(z) by the complex Gauss-Jordan elimination of [zI - Φ | γ] with the family's pivot rule on |z|², the brackets of the
continuous verb on the grid, the bisection of the ARC (mid = (z_lo + z_hi) / |z_lo + z_hi|, one square root and one division) with its end
rule (mid equals an end in both components, or the cap), the same selection, ω* = atan2(Im z*, Re z*) / Ts. Beside it the exact side
(numpy.linalg.solve for L, scipy.optimize.brentq on θ inside the same brackets) and the generators of tests/test_dmargins_host.py and
tests/test_gpu_dmargins.py. Brackets, selection, deviation measure, fairness and the continuous generators are margins_prototype's.

A system is (Φ [nx, nx], γ [nx], c [nx], d). A result is (sel [10], counts [2], all [6, KMAX], status), as fb_lss_dmargins lays out one
system. HALVINGS records the largest number of halvings any bracket took since the module was loaded: the kernel's cap DM_ITERS is the
figure tests/test_dmargins_host.py observes over all its cases, plus 10."""
import functools

import numpy as np

import margins_prototype as mp
from margins_prototype import (FACTOR, FLOOR, FAIR_GRID, FAIR_GM, PROTO_MAX, KMAX, NOT_FINITE, SINGULAR, TRUNCATED, K_CLOSED,  # noqa: F401
                               brackets, deviation, fairness, embed, cube, modes, work_systems, from_device)

ITERS = 63                        # fbw::DM_ITERS
OBSERVED = 53                     # the largest halving count the host test sees over all its cases: ITERS = OBSERVED + 10
HALVINGS = [0]
NX_CLOSED = (2, 7, 8, 9, 16, 17, 31, 32)
K_DELAY = (0.3, 0.5, 0.8)
K_STABILITY = (0.5, 0.9, 1.1, 1.5)      # the closed loop z² - z + K is stable for 0 < K < 1
TS_CLOSED = 0.02
TH_CLOSED = 0.9 * np.pi * np.logspace(-2.0, 0.0, 33)
TS_ZOH = (0.05, 0.2, 0.5)
N_BIG = 130


def circle(w, Ts):
    """what the host hands the device: cos and sin of θ_k = ω_k Ts"""
    th = np.asarray(w, dtype=np.float64) * Ts
    return np.cos(th), np.sin(th)


# ---- L(z) ----------------------------------------------------------------------------------------------------------------------------------
def response(Phi, g, c, d, cz, sz):
    """(c inv(zI - Φ) γ + d, ok) at z = cz + j sz: Gauss-Jordan on the rows of [zI - Φ | γ], the diagonal -Φ_rr + cz in the real part and sz
    in the imaginary part, the pivot of step k the largest |z|² among the rows not yet used, the lowest row at a tie; not ok when that is
    zero or not finite, or the value is not finite"""
    nx = Phi.shape[0]
    Z = np.zeros((nx, nx + 1), dtype=np.complex128)
    Z[:, :nx] = -Phi
    Z[np.arange(nx), np.arange(nx)] = (-np.diag(Phi) + cz) + 1j * sz
    Z[:, nx] = g
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


def exact_response(Phi, g, c, d, z):
    return d + np.dot(c, np.linalg.solve(z * np.eye(Phi.shape[0]) - Phi, g.astype(np.complex128)))


def dfreqresp(Phi, g, c, d, w, Ts):
    """fb_lss_dfreqresp of one system: complex [nw], NaN where the elimination found no pivot"""
    cs, sn = circle(w, Ts)
    out = np.empty(len(cs), dtype=np.complex128)
    for k in range(len(cs)):
        v, ok = response(Phi, g, c, d, cs[k], sn[k])
        out[k] = v if ok else complex(np.nan, np.nan)
    return out


# ---- the contract --------------------------------------------------------------------------------------------------------------------------
def arc_mid(clo, slo, chi, shi):
    """the midpoint of the arc between two points of the upper half circle, and whether it equals an end. The rounding of the division can
    leave the midpoint of two neighbouring points an ulp OUTSIDE them, and then it never equals either: so each component is clamped between
    the ends' where it is monotone along the arc — the cosine always (it falls from 0 to π), the sine where both ends lie on the same side
    of π/2. (A bracket that straddles π/2 to the last ulp ends at the cap.)"""
    mr, mi = clo + chi, slo + shi
    inv = 1.0 / np.sqrt(mr * mr + mi * mi)
    cm, sm = mr * inv, mi * inv
    cm = min(max(cm, min(clo, chi)), max(clo, chi))
    if (clo >= 0.0) == (chi >= 0.0):
        sm = min(max(sm, min(slo, shi)), max(slo, shi))
    return cm, sm, (cm == clo and sm == slo) or (cm == chi and sm == shi)


def margins_z(Phi, g, c, d, cs, sn, w, Ts, gain=1.0):
    """fb_lss_dmargins of one system from the grid's points on the circle (cs, sn) — what the kernel sees; w labels sel[9] only"""
    if not (np.isfinite(Phi).all() and np.isfinite(g).all() and np.isfinite(c).all() and np.isfinite(d) and np.isfinite(gain)):
        return mp._void(NOT_FINITE)
    nw = len(cs)
    L = np.empty(nw, dtype=np.complex128)
    with np.errstate(all="ignore"):
        for k in range(nw):
            v, ok = response(Phi, g, c, d, cs[k], sn[k])
            v = complex(gain * v.real, gain * v.imag)
            if not (ok and np.isfinite(v.real) and np.isfinite(v.imag)):
                return mp._void(SINGULAR)
            L[k] = v
    found, trunc = ([], []), False
    for kind, ks in enumerate(brackets(L)):
        for k in ks:
            if kind == 1 and len(found[1]) == KMAX:     # a gain bracket always counts: nothing to refine
                trunc = True
                break
            clo, slo, chi, shi, llo = cs[k], sn[k], cs[k + 1], sn[k + 1], L[k]
            plo = mp._before(kind, llo)
            it = 0
            while True:
                cm, sm, end = arc_mid(clo, slo, chi, shi)
                if end or it >= ITERS:
                    break
                v, ok = response(Phi, g, c, d, cm, sm)
                if not ok:
                    return mp._void(SINGULAR)
                v = complex(gain * v.real, gain * v.imag)
                it += 1
                if mp._before(kind, v) == plo:
                    clo, slo, llo = cm, sm, v
                else:
                    chi, shi = cm, sm
            HALVINGS[0] = max(HALVINGS[0], it)
            if kind == 0 and not llo.real < 0.0:
                continue
            if len(found[kind]) == KMAX:
                trunc = True
                break
            found[kind].append((np.arctan2(slo, clo) / Ts, llo))
    return mp._finish(L, w, found, trunc)


def margins(Phi, g, c, d, w, Ts, gain=1.0):
    """fb_lss_dmargins of one system"""
    cs, sn = circle(w, Ts)
    return margins_z(Phi, g, c, d, cs, sn, np.asarray(w, dtype=np.float64), Ts, gain)


def exact(Phi, g, c, d, w, Ts, gain=1.0):
    """the exact side: LAPACK for L, Brent's root finder on θ inside the same grid brackets, the same acceptance and selection"""
    from scipy.optimize import brentq
    w = np.asarray(w, dtype=np.float64)
    f = lambda th: gain * exact_response(Phi, g, c, d, complex(np.cos(th), np.sin(th)))
    th = w * Ts
    L = np.array([f(t) for t in th])
    fn = (lambda t: f(t).imag, lambda t: abs(f(t)) ** 2 - 1.0)
    found, trunc = ([], []), False
    for kind, ks in enumerate(brackets(L)):
        for k in ks:
            if len(found[kind]) == KMAX and kind == 1:
                trunc = True
                break
            t = brentq(fn[kind], th[k], th[k + 1], xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)
            v = f(t)
            if kind == 0 and not v.real < 0.0:
                continue
            if len(found[kind]) == KMAX:
                trunc = True
                break
            found[kind].append((t / Ts, v))
    return mp._finish(L, w, found, trunc), L


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def delay_integrator(K):
    """K / (z (z - 1)): an integrator and one sample of delay; Φ has an eigenvalue at 0 and no matrix logarithm"""
    return np.array([[1.0, 0.0], [1.0, 0.0]]), np.array([1.0, 0.0]), np.array([0.0, K]), 0.0


def delay_closed_form(K, Ts):
    """gm, wpc, pm (degrees), wgc of K / (z (z - 1)): L(e^jθ) = K / (2 sin(θ/2)) e^(-j (π/2 + 3θ/2))"""
    thg = 2.0 * np.arcsin(K / 2.0)
    return 1.0 / K, np.pi / 3.0 / Ts, 90.0 - 1.5 * np.degrees(thg), thg / Ts


def dembed(sys, nx, rng, rotate=True):
    """the sampled system among nx states: the extra ones stable (spectral radius 1/2), driven by the input and the plant, unobservable;
    then a random orthogonal change of state — margins_prototype.embed for the unit circle"""
    P0, g0, c0, d = sys
    n0 = P0.shape[0]
    P, g, c = np.zeros((nx, nx)), np.zeros(nx), np.zeros(nx)
    P[:n0, :n0], g[:n0], c[:n0] = P0, g0, c0
    if nx > n0:
        F = rng.standard_normal((nx - n0, nx - n0))
        F *= 0.5 / np.abs(np.linalg.eigvals(F)).max()
        P[n0:, n0:], P[n0:, :n0], g[n0:] = F, rng.standard_normal((nx - n0, n0)), rng.standard_normal(nx - n0)
    if rotate and nx > 1:
        Q = np.linalg.qr(rng.standard_normal((nx, nx)))[0]
        P, g, c = Q @ P @ Q.T, Q @ g, c @ Q.T
    return P, g, c, d


VARIANTS = 4      # distinct changes of state per K: a batch cycles through len(K_DELAY) * VARIANTS systems, 12 never divides its sizes


@functools.lru_cache(maxsize=None)
def closed_systems(nx):
    """the distinct systems of the closed-form batches at this nx, with K of each"""
    rng = np.random.default_rng(2000 + nx)
    return [(dembed(delay_integrator(K), nx, rng), K) for _ in range(VARIANTS) for K in K_DELAY]


W_CLOSED = TH_CLOSED / TS_CLOSED


def zoh(sys, Ts):
    """the zero-order hold of a continuous (A, b, c, d): (Φ, γ, c, d) by the matrix exponential of [[A, b], [0, 0]] Ts"""
    from scipy.linalg import expm
    A, b, c, d = sys
    nx = A.shape[0]
    M = np.zeros((nx + 1, nx + 1))
    M[:nx, :nx], M[:nx, nx] = A, b
    E = expm(M * Ts)
    return E[:nx, :nx].copy(), E[:nx, nx].copy(), c, d


def w_zoh(Ts, nw=33, lo=-2.0):
    """a grid that ends at nine tenths of the Nyquist frequency (L is real at θ = π: no accuracy test goes there)"""
    return np.logspace(lo, np.log10(0.9 * np.pi / Ts), nw)


def edge_grid(K, nw, Ts=TS_CLOSED):
    """a grid whose first interval holds the gain crossing of K / (z (z - 1)) and whose last interval holds its phase crossing"""
    gm, wpc, pm, wgc = delay_closed_form(K, Ts)
    r = (wpc / wgc) ** (1.0 / (nw - 2))           # each crossing at the geometric middle of its interval
    return wgc * r ** (np.arange(nw) - 0.5)


TS_WORK, TS_MODES = 0.01, 0.001
W_WORK = w_zoh(TS_WORK, 161)
W_MODES = np.logspace(-1.0, np.log10(30.0), 257)


def lss_arrays(systems, **kw):
    """margins_prototype.lss_arrays: dict(A, B, C, D, xdot0, x0, u0, y0) [n, ...] with every system's channel at (iu, iy)"""
    return mp.lss_arrays(systems, **kw)
