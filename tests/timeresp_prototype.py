"""The algorithm of fb_lss_stepinfo restated in numpy fp64 (test infrastructure; kernel: csrc/timeresp_kernels.hpp; docs/design/linearize.md,
"Step responses on the device"), the exact side the tests hold it to, the generator of the random plants, the margins of the deciding samples,
and the two loops whose StepInfo tables the reference's robot2d design notebook stores (tests/golden/robot2d_stepinfo.json).

    channel   x' = A x + b, y = c x + d from rest;  samples y_k at t_k = k dt, k = 0 .. N
    prototype the classical RK4 in the steppers' stage form, each row's dot product summed over ascending columns from the row's constant;
              pass 1 (first and last sample, extrema at their first index, blow-up), then y0, yf, dir and stepsize, then pass 2 over the same
              samples (the two first crossings, the last sample outside the settling band). The kernel recomputes the trajectory for pass 2
              bit for bit; here the samples are kept.
    exact     the same samples by scipy.linalg.expm (zero-order hold of the augmented [[A, b], [0, 0]])
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIVERGED, FLAT, NX_MAX = 1, 2, 31          # FB_STEPINFO_* (include/flightbatch.h)
BLOWUP = 1e12
FIELDS = ("y0", "yf", "stepsize", "peak", "peaktime", "overshoot", "undershoot", "settlingtime", "risetime")
DEFAULT_OPTS = (0.02, 0.1, 0.9)            # settling_th, rise_lo, rise_hi

# ---- the GPU tests' cases ---------------------------------------------------------------------------------------------------------------------
SEED = 41
NX_ALL = (1, 7, 8, 15, 16, 31)             # each group size at its smallest nx and at nx = P - 1
NU, NY = 2, 3
N_SYS = 9
CHANNELS = ((0, 0), (1, 1), (0, 2), (1, 1))   # (iu, iy): both inputs, all three outputs, one channel twice
T_SIM, DT = 2.0, 1e-3


def group(nx):
    return 8 if nx + 1 <= 8 else 16 if nx + 1 <= 16 else 32


def samples_count(nsteps, stride):
    return -(-nsteps // stride) + 1


def plants(nx, n=N_SYS, seed=SEED):
    """A [n, nx, nx] = -(L L' + I / 2) + (S - S') with entries ~ N(0, 1 / nx), so A + A' < 0 (tests/pid_prototype.py's stable plants); random
    B [n, nx, NU], C [n, NY, nx], D [n, NY, NU]"""
    rng = np.random.default_rng(seed + 1000 * nx)
    L = rng.standard_normal((n, nx, nx)) / np.sqrt(nx)
    S = rng.standard_normal((n, nx, nx)) / np.sqrt(nx)
    A = -(L @ L.transpose(0, 2, 1) + 0.5 * np.eye(nx)) + (S - S.transpose(0, 2, 1))
    return A, rng.standard_normal((n, nx, NU)), rng.standard_normal((n, NY, nx)), rng.standard_normal((n, NY, NU))


def model(fb, A, B, C, D, x0=None):
    """the plants as a LinearizedSS batch at a zero linearisation point (or at x0 [n, nx])"""
    n, nx = A.shape[:2]
    nu, ny = B.shape[2], C.shape[1]
    z = np.zeros
    return fb.LinearizedSS(xdot0=z((n, nx)), x0=z((n, nx)) if x0 is None else x0, u0=z((n, nu)), y0=z((n, ny)), A=A, B=B, C=C, D=D,
                           x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=tuple(f"u{k}" for k in range(nu)),
                           y_labels=tuple(f"y{k}" for k in range(ny)))


def pairs(A, B, C, D, channels):
    """the channels of every system as pairs in the kernel's order q = j n + i: A [m n, nx, nx], b [m n, nx], c [m n, nx], d [m n]"""
    n = A.shape[0]
    Ap = np.concatenate([A for _ in channels])
    b = np.concatenate([B[:, :, iu] for iu, _ in channels])
    c = np.concatenate([C[:, iy, :] for _, iy in channels])
    d = np.concatenate([D[:, iy, iu] for iu, iy in channels])
    assert Ap.shape[0] == n * len(channels)
    return Ap, b, c, d


# ---- the samples --------------------------------------------------------------------------------------------------------------------------------
def _rows(M, c0, z):
    """c0 + sum_c M[:, :, c] z_c, c ascending (the lanes' dot products)"""
    acc = c0.copy()
    for k in range(M.shape[2]):
        acc = acc + M[:, :, k] * z[:, k:k + 1]
    return acc


def samples_rk4(A, b, c, d, N, dt):
    """y [N + 1, B] of the pairs (A[k], b[k], c[k], d[k]) by RK4 in the steppers' stage form"""
    hdt, dt6 = dt / 2, dt / 6
    B, nx = b.shape
    x = np.zeros((B, nx))
    y = np.empty((N + 1, B))
    c3 = c[:, None, :]
    with np.errstate(all="ignore"):
        for k in range(N):
            y[k] = _rows(c3, d[:, None], x)[:, 0]
            k1 = _rows(A, b, x)
            k2 = _rows(A, b, x + hdt * k1)
            k3 = _rows(A, b, x + hdt * k2)
            k4 = _rows(A, b, x + dt * k3)
            x = x + dt6 * (2 * (k2 + k3) + (k1 + k4))
        y[N] = _rows(c3, d[:, None], x)[:, 0]
    return y


def samples_exact(A, b, c, d, N, dt):
    """the same samples by exact discretisation: expm of the augmented [[A, b], [0, 0]] dt"""
    from scipy.linalg import expm
    B, nx = b.shape
    y = np.empty((N + 1, B))
    for p in range(B):
        aug = np.zeros((nx + 1, nx + 1))
        aug[:nx, :nx] = A[p]; aug[:nx, nx] = b[p]
        E = expm(aug * dt)
        Phi, Gam = E[:nx, :nx], E[:nx, nx]
        x = np.zeros(nx)
        for k in range(N + 1):
            y[k, p] = c[p] @ x + d[p]
            x = Phi @ x + Gam
    return y


def dc_gain(A, b, c, d):
    """d - c inv(A) b of every pair"""
    return np.array([d[p] - c[p] @ np.linalg.solve(A[p], b[p]) for p in range(len(d))])


# ---- StepInfo of one pair ------------------------------------------------------------------------------------------------------------------------
def _pass1(y):
    first, last = y[0], y[-1]
    imx, imn = 0, 0
    mx, mn = -np.inf, np.inf
    for k, v in enumerate(y):
        if v > mx:
            mx, imx = v, k
        if v < mn:
            mn, imn = v, k
    blown = bool((~(np.abs(y) <= BLOWUP)).any())
    return first, last, mx, imx, mn, imn, blown


def _endpoints(y, y0_in, yf_in):
    first, last = y[0], y[-1]
    y0 = first if y0_in is None or np.isnan(y0_in) else y0_in
    yf = last if yf_in is None or np.isnan(yf_in) else yf_in
    with np.errstate(all="ignore"):
        stepsize = abs(yf - y0)
    flat = not (stepsize > 0.0) or not np.isfinite(stepsize)
    down = (not flat) and (yf - y0 < 0.0)
    return y0, yf, stepsize, flat, down


def _pass2(y, y0, yf, stepsize, down, opts):
    th, lo, hi = opts
    dirn = -1.0 if down else 1.0
    lo_t, hi_t, band = lo * stepsize, hi * stepsize, th * stepsize
    e = dirn * (y - y0)
    above_lo, above_hi, outside = np.flatnonzero(e > lo_t), np.flatnonzero(e > hi_t), np.flatnonzero(np.abs(y - yf) > band)
    ilo = int(above_lo[0]) if above_lo.size else -1
    ihi = int(above_hi[0]) if above_hi.size else -1
    iout = int(outside[-1]) if outside.size else -1
    return ilo, ihi, iout


def stepinfo(y, dt, y0_in=None, yf_in=None, opts=DEFAULT_OPTS):
    """(info [9], status, indices (ipeak, iset, ilo, ihi)) of the samples y [N + 1] of one pair"""
    N = len(y) - 1
    first, last, mx, imx, mn, imn, blown = _pass1(y)
    nan = np.nan
    if blown:
        return np.full(9, nan), DIVERGED, (-1, -1, -1, -1)
    y0, yf, stepsize, flat, down = _endpoints(y, y0_in, yf_in)
    with np.errstate(all="ignore"):
        ilo, ihi, iout = _pass2(y, y0, yf, stepsize, down, opts)
        peak, ipeak = (mn, imn) if down else (mx, imx)
        dirn = -1.0 if down else 1.0
        iset = 0 if iout < 0 else min(iout + 1, N)
        info = np.array([y0, yf, stepsize, peak, ipeak * dt, dirn * 100.0 * (peak - yf) / stepsize if not flat else nan,
                         max(0.0, 100.0 * ((mx - y0) if down else (y0 - mn)) / stepsize) if not flat else nan, iset * dt,
                         nan if (ilo < 0 or ihi < 0) else (ihi - ilo) * dt])
    if flat:
        info[5:] = nan
        return info, FLAT, (ipeak, -1, -1, -1)
    return info, 0, (ipeak, iset, ilo, ihi)


def stepinfo_batch(Y, dt, y0_in=None, yf_in=None, opts=DEFAULT_OPTS):
    """info [9, B], status [B] of the samples Y [N + 1, B]"""
    B = Y.shape[1]
    info, status = np.empty((9, B)), np.zeros(B, dtype=np.int32)
    for p in range(B):
        info[:, p], status[p], _ = stepinfo(Y[:, p], dt, None if y0_in is None else y0_in[p], None if yf_in is None else yf_in[p], opts)
    return info, status


def margins(y, y0_in=None, yf_in=None, opts=DEFAULT_OPTS):
    """the distance of every deciding sample of a healthy pair from its threshold, in units of the step size: the two rise crossings and their
    predecessors (or, where a level is never reached, the sample that comes closest), the last sample outside the settling band and its
    successor (or the sample closest to the band's edge, where none is outside), and the gap between the peak and the runner-up extremum
    at another index. A device whose samples differ from these by less than the smallest margin finds the same indices."""
    N = len(y) - 1
    th, lo, hi = opts
    _, _, mx, imx, mn, imn, blown = _pass1(y)
    y0, yf, stepsize, flat, down = _endpoints(y, y0_in, yf_in)
    assert not blown and not flat
    ilo, ihi, iout = _pass2(y, y0, yf, stepsize, down, opts)
    dirn = -1.0 if down else 1.0
    e = dirn * (y - y0)
    out = {}
    for name, idx, level in (("rise_lo", ilo, lo * stepsize), ("rise_hi", ihi, hi * stepsize)):
        if idx < 0:
            out[name] = float(np.min(np.abs(e - level)))
        else:
            out[name] = float(min(abs(e[idx] - level), abs(e[idx - 1] - level) if idx > 0 else np.inf))
    dist = np.abs(np.abs(y - yf) - th * stepsize)
    if iout < 0:
        out["settling"] = float(dist.min())
    else:
        out["settling"] = float(min(dist[iout], dist[iout + 1] if iout < N else np.inf))
    ipeak = imn if down else imx
    others = np.delete(y, ipeak)
    out["peak"] = float(abs(y[ipeak] - (others.min() if down else others.max()))) if others.size else np.inf
    return {k: v / stepsize for k, v in out.items()}


def gpu_variants(P, Y):
    """name -> (y0_in, yf_in, opts) of the runs tests/test_gpu_timeresp.py makes over the pairs P with RK4 samples Y: the defaults; yf given
    as the exact DC gain on the even pairs (NaN, i.e. the last sample, on the odd ones); y0 given a twentieth of the DC step below the
    first sample on two pairs of three; other thresholds"""
    A, b, c, d = P
    B = len(d)
    dc = dc_gain(A, b, c, d)
    yf_in = np.where(np.arange(B) % 2 == 0, dc, np.nan)
    y0_in = np.where(np.arange(B) % 3 != 0, d - 0.05 * (dc - d), np.nan)
    return {"defaults": (None, None, DEFAULT_OPTS), "yf given": (None, yf_in, DEFAULT_OPTS), "y0 given": (y0_in, None, DEFAULT_OPTS),
            "thresholds": (None, None, (0.05, 0.2, 0.8))}


def failure_case():
    """(plants, channels, yf_in [3, 7]) of the failure test: seven plants 1 / (s - a) with three outputs each. System 2 is 1 / (s - 20)
    (every channel diverges), output 1 of system 4 is identically zero (flat), and system 5 is 1 / (s + 0.01) seen through output 0 with
    yf given as its DC gain 100, 90 % of which is out of reach within T_SIM (no rise time)"""
    rng = np.random.default_rng(6)
    a = -rng.uniform(1.0, 4.0, 7)
    a[2], a[5] = 20.0, -0.01
    Cm = rng.uniform(0.5, 2.0, (7, 3, 1))
    D = rng.uniform(0.1, 0.3, (7, 3, 1))
    Cm[4, 1, 0] = D[4, 1, 0] = 0.0
    Cm[5, 0, 0], D[5, 0, 0] = 1.0, 0.0
    yf = np.full((3, 7), np.nan)
    yf[0, 5] = 100.0
    return (a.reshape(7, 1, 1), np.ones((7, 1, 1)), Cm, D), ((0, 0), (0, 1), (0, 2)), yf


def sample_dev(Y, Yref):
    """worst |Y - Yref| per pair, scaled by the pair's max|Yref| [B]"""
    return np.abs(Y - Yref).max(axis=0) / np.abs(Yref).max(axis=0)


# ---- the print format (flightbatch.timeresp.StepInfo.show restated, so that a host test needs no device) ------------------------------------------
def show(info):
    f = lambda v, spec: ("NaN".rjust(5 if spec.startswith("%5") else 0) if np.isnan(v) else spec % v)
    rows = [("Initial value:", f(info[0], "%.3f")), ("Final value:", f(info[1], "%.3f")), ("Step size:", f(info[2], "%.3f")),
            ("Peak:", f(info[3], "%.3f")), ("Peak time:", f(info[4], "%.3f") + " s"), ("Overshoot:", f(info[5], "%5.2f") + " %"),
            ("Undershoot:", f(info[6], "%5.2f") + " %"), ("Settling time:", f(info[7], "%.3f") + " s"), ("Rise time:", f(info[8], "%.3f") + " s")]
    return ["%-19s%s" % r for r in rows]


# ---- the notebook's two loops (tests/golden/robot2d_stepinfo.json) ----------------------------------------------------------------------------------
def stored_tables():
    return json.load(open(os.path.join(GOLDEN, "robot2d_stepinfo.json"), encoding="utf-8"))


def notebook_loops(A, B, k_p=0.6):
    """(A, b, c, d) of v <- v_ref of the LQR velocity loop and of η <- η_ref of the position loop v_ref = k_p (η_ref - η), from the vehicle's
    A [4, 4], B [4, 1] (states ω, v, θ, η) and robot2d.h5's gains: the velocity loop is poles_prototype.velocity_loop's A (states ω, v, θ, η,
    ξ; m = K_fwd v_ref - K_x (ω, v, θ) - ξ, ξ' = K_int (v - v_ref)) with the input column [B K_fwd; -K_int]"""
    from poles_prototype import velocity_loop
    from support import gains_from_h5
    g = gains_from_h5()
    K_fwd, K_int = g[3], g[4]
    Av = velocity_loop(A, B)
    bv = np.concatenate([B[:, 0] * K_fwd, [-K_int]])
    cv = np.array([0.0, 1.0, 0.0, 0.0, 0.0])
    ce = np.array([0.0, 0.0, 0.0, 1.0, 0.0])
    Ap = Av - k_p * np.outer(bv, ce)
    return (Av, bv, cv, 0.0), (Ap, k_p * bv, ce, 0.0)


def notebook_loops_from_golden():
    lin = json.load(open(os.path.join(GOLDEN, "robot2d_linearization.json"), encoding="utf-8"))
    return notebook_loops(np.array(lin["A"]), np.array(lin["B"]))


def loop_model(fb, A, b, c, d, labels=("u", "y")):
    """one channel as a one-input, one-output LinearizedSS of one system"""
    nx = len(b)
    z = np.zeros
    return fb.LinearizedSS(xdot0=z((1, nx)), x0=z((1, nx)), u0=z((1, 1)), y0=z((1, 1)), A=A[None].copy(), B=b[None, :, None].copy(),
                           C=c[None, None, :].copy(), D=np.full((1, 1, 1), d), x_labels=tuple(f"x{k}" for k in range(nx)),
                           u_labels=(labels[0],), y_labels=(labels[1],))


def assert_matches_table(lines, which):
    """`lines` (show's nine) against the stored table, line for line; the second table's peak time is one reference sample short of t_sim
    (the reference's time vector ends at 9.995), so there the value is held to 9.995 within 0.005 instead of to the text"""
    want = stored_tables()[which]["lines"]
    assert len(lines) == len(want) == 9
    for k, (got, ref) in enumerate(zip(lines, want)):
        if which == "position_loop" and k == 4:
            assert got.startswith("Peak time:") and got.endswith(" s") and abs(float(got.split()[2]) - 9.995) <= 0.005 + 1e-12, got
        else:
            assert got == ref, (which, got, ref)
