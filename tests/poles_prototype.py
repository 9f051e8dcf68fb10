"""numpy restatement, one system at a time, of what fbe::k_poles does (flight.jl_amd/csrc/poles_kernels.hpp; docs/design/linearize.md, "Poles
on the device"): the classical dense path, eigenvalues only — Parlett-Reinsch balancing without permutation, Householder reduction to
Hessenberg form, Francis double-shift QR with deflation (EISPACK's balanc / orthes / hqr), then dampreport's order. Every operation is
written in the kernel's order, the group-wide sums included (gsum: the butterfly of the P lanes), so that the kernel and this file differ
in FMA contraction and the <= 1-ulp division only. The GPU tests hold the kernel to LAPACK with a bound derived from this file's own
deviation from LAPACK over the same systems (tests/test_poles_host.py measures it)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NOT_CONVERGED, NOT_FINITE, NX_MAX = 1, 2, 32
BAL_SWEEPS, WINDOW_SWEEPS, BAL_KMAX = 16, 30, 500
NX_ALL = (1, 2, 3, 4, 5, 8, 9, 16, 17, 28, 32)


def group(nx):
    return 8 if nx <= 8 else 16 if nx <= 16 else 32


def gsum(v, P):
    """the sum every lane of a group of P holds after the butterfly v += shfl_xor(v, o), o = P / 2 ... 1 (lanes past len(v) hold 0)"""
    w = np.zeros(P)
    w[:len(v)] = v
    idx = np.arange(P)
    o = P // 2
    while o:
        w = w + w[idx ^ o]
        o //= 2
    return float(w[0])


def balance(a, P):
    """in place: D A inv(D) with D a diagonal of powers of two, at most BAL_SWEEPS sweeps (an exact similarity wherever it stops)"""
    n = a.shape[0]
    for _ in range(BAL_SWEEPS):
        changed = False
        for i in range(n):
            off = np.arange(n) != i
            c = gsum(np.where(off, np.abs(a[:, i]), 0.0), P)
            r = gsum(np.where(off, np.abs(a[i, :]), 0.0), P)
            if not (c > 0.0 and r > 0.0 and np.isfinite(c) and np.isfinite(r)):
                continue
            # the k with r / 2 <= 4^k c < 2 r, from the exponents: no loop whose trip count the data sets
            ec, er = int(np.frexp(c)[1]), int(np.frexp(r)[1])
            k = min(max((er - ec) >> 1, -BAL_KMAX), BAL_KMAX)
            c2 = float(np.ldexp(c, 2 * k))
            if c2 < 0.5 * r and k < BAL_KMAX:
                k += 1
                c2 = 4.0 * c2
            f, fi = float(np.ldexp(1.0, k)), float(np.ldexp(1.0, -k))
            if (c2 + r) * fi < 0.95 * (c + r):
                changed = True
                a[i, off] = a[i, off] * fi
                a[off, i] = a[off, i] * f
        if not changed:
            break
    return a


def hessenberg(a, P):
    """in place: Householder reflections, column m - 1 at step m; a zero column is skipped, its bits left alone"""
    n = a.shape[0]
    for m in range(1, n - 1):
        col = np.where(np.arange(n) >= m, a[:, m - 1], 0.0)
        scale = gsum(np.abs(col), P)
        if not scale > 0.0:     # (zero, or NaN: nothing to reflect)
            continue
        o = col / scale
        h = gsum(o * o, P)
        g = -float(np.copysign(np.sqrt(h), o[m]))
        h = h - o[m] * g
        o[m] = o[m] - g
        f = np.zeros(n)                     # lane j: v' A[:, j], rows ascending
        for i in range(m, n):
            f = f + o[i] * a[i, :]
        f = f / h
        for i in range(m, n):
            a[i, m:] = a[i, m:] - f[m:] * o[i]
        f = np.zeros(n)                     # lane i: A[i, :] v, columns ascending
        for j in range(m, n):
            f = f + o[j] * a[:, j]
        f = f / h
        for j in range(m, n):
            a[:, j] = a[:, j] - f * o[j]
        a[m, m - 1] = scale * g
        a[m + 1:, m - 1] = 0.0
    return a


def _sign(x, s):
    return float(np.copysign(x, s))


def hqr(a, P):
    """eigenvalues of the Hessenberg matrix a (destroyed): (wr, wi, sweeps, status), poles in the position the elimination leaves them"""
    n = a.shape[0]
    wr, wi = np.zeros(n), np.zeros(n)
    colsum = np.zeros(n)
    for i in range(n):                      # lane j: sum of |a[i, j]| over the Hessenberg part of column j, rows ascending
        colsum = colsum + np.where(np.arange(n) >= i - 1, np.abs(a[i, :]), 0.0)
    anorm = gsum(colsum, P)
    nn, t, its, sweeps = n - 1, 0.0, 0, 0
    while nn >= 0:
        l = 0
        for i in range(nn, 0, -1):
            s = abs(a[i - 1, i - 1]) + abs(a[i, i])
            if s == 0.0:
                s = anorm
            if abs(a[i, i - 1]) + s == s:
                l = i
                break
        if l > 0:
            a[l, l - 1] = 0.0
        x = a[nn, nn]
        if l == nn:
            wr[nn], wi[nn] = x + t, 0.0
            nn -= 1; its = 0
            continue
        y = a[nn - 1, nn - 1]
        w = a[nn, nn - 1] * a[nn - 1, nn]
        if l == nn - 1:
            p = 0.5 * (y - x)
            q = p * p + w
            z = float(np.sqrt(abs(q)))
            x = x + t
            if q >= 0.0:
                z = p + _sign(z, p)
                wr[nn - 1] = wr[nn] = x + z
                if z != 0.0:
                    wr[nn] = x - w / z
                wi[nn - 1] = wi[nn] = 0.0
            else:
                wr[nn - 1] = wr[nn] = x + p
                wi[nn - 1], wi[nn] = z, -z
            nn -= 2; its = 0
            continue
        if its == WINDOW_SWEEPS:
            return wr, wi, sweeps, NOT_CONVERGED
        if its in (10, 20):
            t = t + x
            for i in range(nn + 1):
                a[i, i] = a[i, i] - x
            s = abs(a[nn, nn - 1]) + abs(a[nn - 1, nn - 2])
            x = y = 0.75 * s
            w = -0.4375 * s * s
        its += 1; sweeps += 1
        for m in range(nn - 2, l - 1, -1):
            z = a[m, m]
            r = x - z
            s = y - z
            p = (r * s - w) / a[m + 1, m] + a[m, m + 1]
            q = a[m + 1, m + 1] - z - r - s
            r = a[m + 2, m + 1]
            s = abs(p) + abs(q) + abs(r)
            p, q, r = p / s, q / s, r / s
            if m == l:
                break
            u = abs(a[m, m - 1]) * (abs(q) + abs(r))
            v = abs(p) * (abs(a[m - 1, m - 1]) + abs(z) + abs(a[m + 1, m + 1]))
            if u + v == v:
                break
        for k in range(m, nn):
            last = k == nn - 1
            if k != m:
                p, q, r = a[k, k - 1], a[k + 1, k - 1], (0.0 if last else a[k + 2, k - 1])
                x = abs(p) + abs(q) + abs(r)
                if not x != 0.0:
                    continue
                p, q, r = p / x, q / x, r / x
            s = _sign(float(np.sqrt(p * p + q * q + r * r)), p)
            if k == m:
                if l != m:
                    a[k, k - 1] = -a[k, k - 1]
            else:
                a[k, k - 1] = -s * x
                a[k + 1, k - 1] = 0.0
                if not last:
                    a[k + 2, k - 1] = 0.0
            p = p + s
            x, y, z = p / s, q / s, r / s
            q, r = q / p, r / p
            j = slice(k, nn + 1)            # lane j of columns k ... nn
            pp = a[k, j] + q * a[k + 1, j]
            if not last:
                pp = pp + r * a[k + 2, j]
                a[k + 2, j] = a[k + 2, j] - pp * z
            a[k + 1, j] = a[k + 1, j] - pp * y
            a[k, j] = a[k, j] - pp * x
            i = slice(l, min(nn, k + 3) + 1)   # lane i of rows l ... min(nn, k + 3)
            pp = x * a[i, k] + y * a[i, k + 1]
            if not last:
                pp = pp + z * a[i, k + 2]
                a[i, k + 2] = a[i, k + 2] - pp * r
            a[i, k + 1] = a[i, k + 1] - pp * q
            a[i, k] = a[i, k] - pp
    return wr, wi, sweeps, 0


def sort_poles(wr, wi):
    """ascending by |pole|, then Re, then Im, then position: every pole counts those that precede it and goes to that rank"""
    n = len(wr)
    wn = np.sqrt(wr * wr + wi * wi)
    out_r, out_i = np.empty(n), np.empty(n)
    for k in range(n):
        rank = 0
        for j in range(n):
            if j == k:
                continue
            before = (wn[j] < wn[k] or (wn[j] == wn[k] and (wr[j] < wr[k] or (wr[j] == wr[k] and (wi[j] < wi[k] or (wi[j] == wi[k] and j < k))))))
            rank += bool(before)
        out_r[rank], out_i[rank] = wr[k], wi[k]
    return out_r, out_i


def poles(A, balancing=True, full=False):
    """(poles complex128 [nx], sweeps, status) of one system; with `full`, also the balanced matrix the iteration started from"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    P = group(n)
    nan = np.full(n, np.nan + 1j * np.nan)
    if not np.isfinite(A).all():
        return (nan, 0, NOT_FINITE, None) if full else (nan, 0, NOT_FINITE)
    a = A.copy()
    if balancing:
        balance(a, P)
    bal = a.copy()
    hessenberg(a, P)
    with np.errstate(all="ignore"):
        wr, wi, sweeps, status = hqr(a, P)
    if status == 0 and not (np.isfinite(wr).all() and np.isfinite(wi).all()):
        status = NOT_FINITE
    if status:
        lam = nan
    else:
        sr, si = sort_poles(wr, wi)
        lam = sr + 1j * si
    return (lam, sweeps, status, bal) if full else (lam, sweeps, status)


def poles_batch(A, balancing=True):
    out = [poles(a, balancing) for a in A]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32), np.array([o[2] for o in out], dtype=np.int32)


# ---- what the tests share

def systems(nx, n=130):
    """the generator of the issue's preconditions: eigenvalue condition numbers <= 147, gaps >= 8.7e-3 of max|pole|"""
    return np.random.default_rng(100 + nx).standard_normal((n, nx, nx)) / np.sqrt(nx)


def badly_scaled():
    """(A, D A inv(D)) with D = 2^k, k in [-20, 20): without balancing the second loses six digits"""
    rng = np.random.default_rng(5)
    A = rng.standard_normal((16, 16)) / 4
    d = 2.0 ** rng.integers(-20, 20, 16)
    return A, (d[:, None] * A) / d[None, :]


def match_dev(lam, mu):
    """worst matched distance / max|mu| under the assignment that minimises the total distance"""
    from scipy.optimize import linear_sum_assignment
    lam, mu = np.asarray(lam), np.asarray(mu)
    if not np.isfinite(lam).all():
        return np.inf
    d = np.abs(lam[:, None] - mu[None, :])
    r, c = linear_sum_assignment(d)
    return float(d[r, c].max() / max(np.abs(mu).max(), np.finfo(float).tiny))


def batch_dev(L, M):
    return max(match_dev(l, m) for l, m in zip(L, M))


def sort_rule_holds(lam):
    """ascending |pole| (to 4 ulp: the device's sqrt(re^2 + im^2) is not numpy's hypot), and among bitwise-equal |pole| ascending (Re, Im)"""
    wn = np.abs(lam)
    for a, b, wa, wb in zip(lam[:-1], lam[1:], wn[:-1], wn[1:]):
        if wb < wa * (1 - 4 * np.finfo(float).eps):
            return False
        if wa == wb and (b.real, b.imag) < (a.real, a.imag):
            return False
    return True


def exact_cases():
    """(A, the poles in the sorted order), every value exact"""
    tri = np.triu(np.arange(1.0, 26.0).reshape(5, 5) / 8) * np.array([1, -1, 1, -1, 1.0])[None, :]
    return [
        (np.zeros((3, 3)), np.zeros(3) + 0j),
        (np.eye(4, k=1), np.zeros(4) + 0j),
        (np.array([[0.0, 1.0], [-1.0, 0.0]]), np.array([-1j, 1j])),
        (np.array([[0.0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 2], [0, 0, -2, 0]]), np.array([0, 0, -2j, 2j])),
        (np.diag([3.0, -1.0, 0.5, -0.5, 7.0, 1.0]), np.array([-0.5, 0.5, -1.0, 1.0, 3.0, 7.0]) + 0j),
        (tri, np.array(sorted(np.diag(tri), key=lambda v: (abs(v), v))) + 0j),
    ]


def damp_row(lam):
    """dampreport's figures for one pole: (wn, zeta, tau) — zeta = -cos(arg pole), so -1 for a pole at +0; tau = -1 / Re"""
    wn = abs(lam)
    zeta = -np.cos(np.angle(lam))
    with np.errstate(divide="ignore"):
        tau = -1.0 / np.float64(lam.real)
    return wn, zeta, tau


# ---- the two tables the reference's robot2d design notebook stores (tests/golden/robot2d_dampreport.json) -----------------------------
def notebook_systems():
    """(A of Robot2D.Vehicle as the notebook prints it, A of the velocity loop with robot2d.h5's gains), states (ω, v, θ, η) and (ω, v, θ, η, ξ)"""
    lin = json.load(open(os.path.join(GOLDEN, "robot2d_linearization.json"), encoding="utf-8"))
    A, B = np.array(lin["A"]), np.array(lin["B"])
    return A, velocity_loop(A, B)


def velocity_loop(A, B):
    """A_cl = [[A - B [K_x 0], -B], [K_xi C_v, 0]] as the notebook's `connect` wires it: m = m_fwd - K_x (ω, v, θ) - ξ, ξ' = K_int (v - v_ref)"""
    from support import gains_from_h5
    g = gains_from_h5()
    K_x, K_int = g[0:3], g[4]
    Kfull = np.concatenate([K_x, [0.0]])[None, :]
    Cv = np.array([[0.0, 1.0, 0.0, 0.0]])
    return np.block([[A - B @ Kfull, -B], [K_int * Cv, np.zeros((1, 1))]])


def table_rows(name):
    d = json.load(open(os.path.join(GOLDEN, "robot2d_dampreport.json"), encoding="utf-8"))
    rows = [[c.strip() for c in line.strip("|").split("|")] for line in d[name]]
    return d["header"], d[name], rows


def half_last_digit(text):
    """half a unit of the last printed digit of a number printed with 3 significant digits"""
    t = text.lstrip("+-")
    return 0.5 * 10.0 ** (-len(t.split(".")[1]) if "." in t else 0)


def assert_matches_table(lam, name):
    """every pole within half a unit of its last printed digit (the pole at zero: |pole| <= 1e-9); damping ratio, frequency and time constant
    as printed, -1 and -Inf for the pole at +0 included"""
    from flightbatch.poles import _g3
    _, _, rows = table_rows(name)
    assert len(lam) == len(rows)
    for l, (pole, zeta, wn, hz, tau) in zip(lam, rows):
        assert l.imag == 0.0
        if pole == "+0":
            assert abs(l) <= 1e-9, l
            continue                     # (its sign, and with it the printed -1 and -Inf, is rounding's: report_with_zero_snapped holds dampreport's text on +0)
        assert abs(l.real - float(pole)) <= half_last_digit(pole), (l, pole)
        w_, z_, t_ = damp_row(l)
        assert (_g3(z_), _g3(w_), _g3(w_ / (2 * np.pi)), _g3(t_)) == (zeta, wn, hz, tau), (l, rows)
    w_, z_, t_ = damp_row(complex(0.0, 0.0))
    assert (_g3(z_), _g3(w_), _g3(w_ / (2 * np.pi)), _g3(t_)) == ("-1", "0", "0", "-Inf")


def report_with_zero_snapped(fb, lam):
    """dampreport's text with a pole of |pole| <= 1e-9 put at +0, where the notebook's LAPACK happened to leave it"""
    lam = np.where(np.abs(lam) <= 1e-9, 0.0 + 0.0j, lam)
    order = np.lexsort((lam.imag, lam.real, np.abs(lam)))
    res = fb.PolesResult(poles=lam[order][None, :], iters=np.zeros(1, np.int32), status=np.zeros(1, np.int32))
    return fb.dampreport(res, 0).split("\n")
