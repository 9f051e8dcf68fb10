"""fb_lss_dlqr (flightbatch.dlqr): the discrete LQR of a batch of sampled models on the device, pinned by

  1. scipy.linalg.solve_discrete_are on random systems on both sides of the 8 | 9 group edge, at nx = 16, nu = 1 and 8, two sample times and a
     single, a ragged and a multi-block batch, through the numpy restatement of the kernel (tests/dlqr_prototype.py; tests/test_dlqr_host.py
     holds the prototype itself to scipy first and checks that the cases are fair);
  2. position independence and repeatability, bit for bit, with groups of one wave that double a different number of times;
  3. the three systems without a stabilising solution and a NaN model, flagged in place among healthy neighbours;
  4. the closed world: its blocks, what is copied bit for bit, the source left as it was;
  5. the optimal-cost identity sum (dx' Q dx + u' R u) = dx0' X dx0 on the device's own stepper;
  6. the continuous limit: dlqr(c2d(w, Ts), Ts Q, Ts R) against fb_lqr(w, Q, R), as far apart as scipy's two solvers say;
  7. the refusals of the C ABI on a live device.

Worlds are made as continuous LinearWorlds and passed through fb.c2d; the reference side designs on the Phi and Gamma read back from the
device (fb_lss_get_model), so c2d's own error is not mixed in.

The shared bound (the family's rule): the device differs from the prototype in FMA contraction and <= 1-ulp division only, so it may deviate
from scipy ten times as far as the prototype does over the same systems, with a floor of 1e-11, every block scaled by its largest entry;
the residual ten times the prototype's, floor 1e-13.

Measured on one MI355X (docs/design/linearize.md, "Discrete LQR on the device", has the table per shape): over the 54 cases of test 1, K and X
within 1.1e-10 of scipy's where the prototype is within 1.1e-10 ((4, 1) at Ts = 0.02: scipy's own error), device against prototype within
2.1e-12, resid <= 4.0e-13, the prototype's count of doublings on every system; the cost identity within 1.2e-13 (prototype 1.5e-13); the
continuous limit 3.2167e-2, 1.6230e-2, 8.1517e-3, equal to scipy's within 1.3e-11."""
import ctypes as C

import numpy as np
import pytest

import c2d_prototype as c2d
import dlqr_prototype as proto
import lqr_prototype as lq
from support import clock

pytestmark = pytest.mark.gpu
FLOOR, MARGIN, RESID_FLOOR, NMAX = proto.FLOOR, proto.MARGIN, proto.RESID_FLOOR, proto.NMAX
FIELDS = ("K", "X", "resid", "iters", "status")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_design(p, q, sel=slice(None)):
    return all(np.array_equal(getattr(p, k), getattr(q, k)[sel], equal_nan=True) for k in FIELDS) and _same(p.K, q.K[sel]) and _same(p.X, q.X[sel])


def _sampled(fb, A, B, Ts, x0=None):
    """the sampled world of design_model(A, B) plants (C = I): made continuous, passed through fb.c2d"""
    src = fb.LinearWorld(fb.design_model(A, B, x0=x0))
    res = fb.c2d(src, Ts)
    src.close()
    return res.world, res.status


def _design(fb, A, B, Ts, Q, R):
    w, st = _sampled(fb, A, B, Ts)
    res = fb.dlqr(w, Q, R)
    Phi, Gam = w.model()
    w.close()
    return res, Phi, Gam, st


_REF = {}


def _reference(fb, nx, nu, Ts):
    """the 130 systems of one shape at one sample time (tests/dlqr_prototype.py, batch: why they are nine systems repeated): Phi and Gamma as
    the device holds them, the prototype's and scipy's designs on them (computed once, read only)"""
    if (nx, nu, Ts) not in _REF:
        A, B, Q, R = proto.batch(nx, nu, NMAX)
        w, st = _sampled(fb, A, B, Ts)
        assert (st == 0).all()
        Phi, Gam = w.model()
        w.close()
        idx, nd = np.arange(NMAX) % proto.N_DISTINCT, proto.N_DISTINCT
        assert _same(Phi, Phi[:nd][idx]) and _same(Gam, Gam[:nd][idx])          # (a repeated system is the same system: designed once on the host)
        pr, Ks, Xs = proto.designs(Phi[:nd], Gam[:nd], Q, R)
        out = (A, B, Q, R, Phi, Gam, {k: v[idx] for k, v in pr.items()}, Ks[idx], Xs[idx])
        for a in (*out[:6], *out[6].values(), *out[7:]):
            a.setflags(write=False)
        _REF[nx, nu, Ts] = out
    return _REF[nx, nu, Ts]


# ---- 1. every shape, sample time and batch edge against scipy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, NMAX])
@pytest.mark.parametrize("Ts", proto.TS_ALL)
@pytest.mark.parametrize("nx,nu", proto.SHAPES)
def test_random_systems_against_scipy(fb, nx, nu, Ts, n, capsys):
    A, B, Q, R, Phi, Gam, pr, Ks, Xs = _reference(fb, nx, nu, Ts)
    res, Phi_n, Gam_n, st = _design(fb, A[:n], B[:n], Ts, Q, R)
    assert (st == 0).all() and _same(Phi_n, Phi[:n]) and _same(Gam_n, Gam[:n])          # the same systems as the reference side's
    assert res.K.shape == (n, nu, nx) and res.X.shape == (n, nx, nx) and res.resid.shape == res.iters.shape == res.status.shape == (n,)
    dK, dX = proto.rel_dev(res.K, Ks[:n]), proto.rel_dev(res.X, Xs[:n])
    pK, pX = proto.rel_dev(pr["K"][:n], Ks[:n]), proto.rel_dev(pr["X"][:n], Xs[:n])
    qK, qX = proto.rel_dev(res.K, pr["K"][:n]), proto.rel_dev(res.X, pr["X"][:n])
    di = np.abs(res.iters.astype(int) - pr["iters"][:n]).max()
    with capsys.disabled():
        print(f"\n[fb_lss_dlqr vs scipy] ({nx:2d}, {nu}) Ts {Ts:g} x {n:3d}: K {dK:.2e} (prototype {pK:.2e}; device vs prototype {qK:.2e})  X {dX:.2e} ({pX:.2e}; {qX:.2e})  "
              f"resid <= {res.resid.max():.2e} ({pr['resid'][:n].max():.2e})  doublings {res.iters.min()} - {res.iters.max()} (|device - prototype| <= {di})  "
              f"status {np.unique(res.status)}", end="")
    assert (res.status == 0).all() and res.success.all() and (pr["status"][:n] == 0).all()
    assert np.array_equal(res.iters, pr["iters"][:n])
    assert dK <= max(MARGIN * pK, FLOOR) and dX <= max(MARGIN * pX, FLOOR)
    assert qK <= max(MARGIN * pK, FLOOR) and qX <= max(MARGIN * pX, FLOOR)
    assert res.resid.max() <= max(MARGIN * pr["resid"][:n].max(), RESID_FLOOR)
    assert np.array_equal(res.X, res.X.transpose(0, 2, 1))


# ---- 2. position, repeatability, different counts of doublings in one wave -----------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(8, 2), (9, 8), (16, 4)])
def test_bitwise_independent_of_position_and_repeatable(fb, nx, nu):
    A, B, Q, R = lq.systems(nx, nu, NMAX)
    w, _ = _sampled(fb, A, B, 0.25)
    big = fb.dlqr(w, Q, R)
    again = fb.dlqr(w, Q, R)
    w.close()
    assert (big.status == 0).all() and _same_design(again, big)
    for n in (1, 3, 9, 63):
        assert _same_design(_design(fb, A[:n], B[:n], 0.25, Q, R)[0], big, slice(0, n)), n
    assert _same_design(_design(fb, A[::-1], B[::-1], 0.25, Q, R)[0], big, slice(None, None, -1))


@pytest.mark.parametrize("nx", [8, 9, 16])
def test_neighbouring_groups_double_a_different_number_of_times(fb, nx, capsys):
    M = c2d.scaled(nx, 2)          # one plant with A times 1, 8, 64, 1, 8, ... before c2d
    Q, R = np.eye(nx), np.eye(2)
    got, Phi, Gam, st = _design(fb, M[4], M[5], 0.25, Q, R)
    want = proto.dlqr_batch(Phi, Gam, Q, R)
    with capsys.disabled():
        print(f"\n[fb_lss_dlqr, one plant times 1, 8, 64] nx {nx}: doublings {got.iters.tolist()}", end="")
    assert (st == 0).all() and (got.status == 0).all() and np.array_equal(got.iters, want["iters"]) and len(set(got.iters[:3].tolist())) == 3
    for i in range(M[4].shape[0]):
        assert _same_design(_design(fb, M[4][[i]], M[5][[i]], 0.25, Q, R)[0], got, [i]), i


# ---- 3. failures in place ------------------------------------------------------------------------------------------------------------------------------
def test_systems_without_a_solution_are_flagged_in_place(fb):
    """66 (3, 1) systems, 5, 64 and 65 replaced by tests/lqr_prototype.py's three systems without a stabilising solution, embedded as
    test_gpu_lqr.py embeds them, sampled at Ts = 0.25. The unstable, uncontrollable mode of the first doubles until the arithmetic overflows;
    the second's integrator and the third's oscillator sit on the unit circle where neither the weights see them nor the input reaches them:
    H converges, A never shrinks, and the bound on the doublings is what ends them. The inputs are fixed and nothing is retried."""
    A, B, Q, R, where, want = proto.failure_case()
    w, st = _sampled(fb, A, B, 0.25)
    assert (st == 0).all()
    Phi, Gam = w.model()
    n = A.shape[0]
    K, X = np.empty(3 * n), np.empty(9 * n)
    resid, iters, status = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = fb.lib.fb_lss_dlqr(w._h, pd(np.asfortranarray(Q).reshape(-1, order="F")), pd(R.reshape(-1)), pd(K), pd(X), pd(resid), pi(iters), pi(status), None)
    assert rc == 0, fb.lib.fb_last_error()
    res = fb.dlqr(w, Q, R, closed=True)
    w.close()
    assert np.array_equal(res.status, status) and np.array_equal(res.K.transpose(2, 1, 0).reshape(-1), K, equal_nan=True) and np.array_equal(res.iters, iters)
    expect = np.zeros(n, dtype=np.int32)
    expect[list(where)] = want
    assert np.array_equal(res.status, expect), res.status
    for i in where:
        p = proto.dlqr(Phi[i], Gam[i], Q, R)
        assert (p["status"], p["iters"]) == (res.status[i], res.iters[i]), (i, p["status"], p["iters"], res.iters[i])
    assert res.iters[64] == res.iters[65] == proto.MAX_ITERS
    ok = expect == 0
    assert np.isnan(res.K[~ok]).all() and np.isnan(res.X[~ok]).all() and np.isnan(res.resid[~ok]).all() and np.array_equal(res.success, ok)
    assert np.isfinite(res.K[ok]).all() and np.isfinite(res.X[ok]).all() and np.isfinite(res.resid[ok]).all()
    # the closed world: NaN where there is a status, and only there; what is copied is copied for every system
    Pc, Gc = res.world.model()
    Cc, Dc = res.world.model_cd()
    res.world.close()
    assert np.isnan(Pc[~ok]).all() and np.isnan(Cc[~ok]).all() and np.isfinite(Pc[ok]).all() and np.isfinite(Cc[ok]).all()
    assert _same(Gc, Gam) and _same(Dc, np.zeros((n, 3, 1)))
    healthy, *_ = _design(fb, A[ok], B[ok], 0.25, Q, R)
    assert (healthy.status == 0).all() and _same_design(healthy, res, ok)
    # a NaN in A before c2d: Phi is NaN, the first solve has no pivot
    A2 = A[:9].copy()
    A2[4, 1, 0] = np.nan
    bad, Phi2, _, st2 = _design(fb, A2, B[:9], 0.25, Q, R)
    assert st2.tolist() == [0, 0, 0, 0, c2d.NOT_FINITE, 0, 0, 0, 0] and np.isnan(Phi2[4]).all()
    assert bad.status[4] == proto.SINGULAR and bad.iters[4] == 1 and np.isnan(bad.K[4]).all() and np.isnan(bad.X[4]).all() and np.isnan(bad.resid[4])
    keep = [0, 1, 2, 3, 6, 7, 8]          # (5 is the first system without a solution)
    assert _same_design(_design(fb, A[keep], B[keep], 0.25, Q, R)[0], bad, keep)


# ---- 4. the closed world -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(5, 2), (9, 8), (16, 4)])
def test_the_closed_world(fb, nx, nu, capsys):
    n, Ts = 9, 0.25
    M = c2d.plants(nx, nu, n)          # offsets, C and D of their own
    _, _, Q, R = lq.systems(nx, nu, 1)
    src = fb.LinearWorld(c2d.model(fb, M))
    w = fb.c2d(src, Ts).world
    src.close()
    rng = np.random.default_rng(nx)
    w.set_state(rng.standard_normal((nx, n)))
    w.u = rng.standard_normal((nu, n))
    w.step(7)
    w.sync()
    snap = lambda: (w.x, w.u, *clock(fb, w), w.status, *w.model(), *w.model_cd(), w.params.dt, w.Ts)
    before = snap()
    res = fb.dlqr(w, Q, R, closed=True)
    after = snap()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[3] == 7 and (res.status == 0).all()
    cw = res.world
    assert cw.Ts == Ts and cw.params.dt == Ts and clock(fb, cw) == (0.0, 0) and (cw.n, cw.nx, cw.nu, cw.ny) == (w.n, w.nx, w.nu, w.ny)
    assert (cw.x_labels, cw.u_labels, cw.y_labels) == (w.x_labels, w.u_labels, w.y_labels)
    Phi, Gam = w.model()
    Cm, D = w.model_cd()
    Pc, Gc = cw.model()
    Cc, Dc = cw.model_cd()
    Ph, Ch = proto.closed(Phi, Gam, Cm, D, res.K)
    dP, dC = float(c2d.block_dev(Pc, Ph).max()), float(c2d.block_dev(Cc, Ch).max())
    with capsys.disabled():
        print(f"\n[fb_lss_dlqr, closed] ({nx:2d}, {nu}) x {n}: Phi - Gam K {dP:.2e}, C - D K {dC:.2e} of the block's largest entry against the host's from the returned K", end="")
    assert dP <= FLOOR and dC <= FLOOR          # (the host's products are exact to rounding: the prototype's deviation is zero, the floor is the bound)
    assert _same(Gc, Gam) and _same(Dc, D) and _same(cw.x.T, M[1]) and _same(cw.u.T, M[2])
    cw.f_ode()
    assert _same(cw.y.T, M[3])
    # delta: one step from the design point of the source's own fresh sampled world and of the closed one (every product is one with an exact zero)
    src = fb.LinearWorld(c2d.model(fb, M))
    fresh = fb.c2d(src, Ts).world
    src.close()
    for v in (fresh, cw):
        v.step(1)
        v.sync()
    assert _same(cw.x, fresh.x) and clock(fb, cw) == (Ts, 1)
    fresh.close()
    si = fb.stepinfo(cw, [(0, 0)], 40 * Ts)
    assert si.ok.all() and si.dt == Ts
    again = fb.dlqr(w, Q, R, closed=True)          # the closed world is a function of the source's model alone
    assert _same(again.world.model()[0], Pc) and _same(again.world.model_cd()[0], Cc) and _same_design(again, res)
    again.world.close()
    cw.close()
    w.close()


# ---- 5. the optimal-cost identity on the device's own stepper --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", proto.COST_SHAPES)
def test_the_cost_of_the_designed_loop_is_x_prime_X_x(fb, nx, nu, capsys):
    n, Ts = proto.COST_N, proto.COST_TS
    A, B, Q, R = lq.systems(nx, nu, n)
    rng = np.random.default_rng(nx)
    dx0 = rng.standard_normal((n, nx))          # (tests/test_dlqr_host.py draws the same)
    x0 = rng.standard_normal((n, nx))
    w, st = _sampled(fb, A, B, Ts, x0=x0)
    Phi, Gam = w.model()
    res = fb.dlqr(w, Q, R, closed=True)
    w.close()
    assert (st == 0).all() and (res.status == 0).all()
    pr, Ks, Xs = proto.designs(Phi, Gam, Q, R)
    radius = max(proto.rho(Phi[i] - Gam[i] @ Ks[i]) for i in range(n))
    M = int(np.ceil(17.0 / -np.log(radius)))
    assert radius <= 0.992 and M < 2200
    cw = res.world
    cw.log_configure(every=1, capacity=M, x=range(nx))
    cw.set_state((x0 + dx0).T)
    cw.step(M)
    cw.sync()
    t, data = cw.log_read()
    cw.close()
    assert data.shape == (M, nx, n) and t[-1] == pytest.approx(M * Ts, rel=1e-12)
    dx = np.concatenate([dx0[None], data.transpose(0, 2, 1) - x0[None]])          # [M + 1, n, nx]: the samples 0 .. M
    J = np.zeros(n)
    for k in range(M):
        J = J + proto.stage_cost(dx[k], res.K, Q, R)
    want = np.einsum("ni,nij,nj->n", dx0, res.X, dx0)
    q, end = np.abs(J - want) / want, np.abs(dx[M]).max(axis=1) / np.abs(dx0).max(axis=1)
    Jp, wantp, endp = proto.cost(Phi, Gam, Q, R, pr["K"], pr["X"], dx0, M)
    qp = np.abs(Jp - wantp) / wantp
    with capsys.disabled():
        print(f"\n[fb_lss_dlqr, optimal cost] ({nx:2d}, {nu}) x {n}, Ts {Ts}, rho <= {radius:.4f}, {M} samples on the device: |sum - dx0' X dx0| / (dx0' X dx0) <= {q.max():.2e} "
              f"(prototype {qp.max():.2e}); |dx_M| / |dx0| <= {end.max():.2e} ({endp.max():.2e})", end="")
    assert q.max() <= max(MARGIN * qp.max(), FLOOR)
    assert end.max() <= max(MARGIN * endp.max(), FLOOR)


# ---- 6. the continuous limit ---------------------------------------------------------------------------------------------------------------------------------
def test_the_continuous_limit(fb, capsys):
    n = 3
    A, B, Q, R = lq.systems(5, 2, n)
    w = fb.LinearWorld(fb.design_model(A, B))
    Kc = fb.lqr(w, Q, R).K
    Kc_p, Kc_s = lq.lqr_batch(A, B, Q, R)["K"], lq.scipy_batch(A, B, Q, R)[0]
    d, dp, ds = [], [], []
    for Ts in proto.LIMIT_TS:
        s = fb.c2d(w, Ts).world
        Phi, Gam = s.model()
        res = fb.dlqr(s, Ts * Q, Ts * R)
        s.close()
        assert (res.status == 0).all()
        d.append(proto.rel_dev(res.K, Kc))
        dp.append(proto.rel_dev(proto.dlqr_batch(Phi, Gam, Ts * Q, Ts * R)["K"], Kc_p))
        ds.append(proto.rel_dev(proto.scipy_batch(Phi, Gam, Ts * Q, Ts * R)[0], Kc_s))
    w.close()
    with capsys.disabled():
        print(f"\n[fb_lss_dlqr, the continuous limit] (5, 2) x {n}: |K_d(Ts Q, Ts R) - K_c| / max|K_c| at Ts {proto.LIMIT_TS}: device " + ", ".join(f"{v:.4e}" for v in d)
              + "; scipy " + ", ".join(f"{v:.4e}" for v in ds) + "; |device - scipy| " + ", ".join(f"{abs(a - b):.1e}" for a, b in zip(d, ds))
              + " (prototype " + ", ".join(f"{abs(a - b):.1e}" for a, b in zip(dp, ds)) + ")", end="")
    for a, p, s in zip(d, dp, ds):
        assert abs(a - s) <= max(MARGIN * abs(p - s), FLOOR)
    assert 2e-2 <= d[0] <= 4e-2 and all(1.7 <= d[k] / d[k + 1] <= 2.3 for k in range(2))          # first order in Ts (tests/test_dlqr_host.py: scipy's say so)


# ---- 7. refusals on a live device --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 4
    rng = np.random.default_rng(7)
    pd = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def dlqr(h, Q, R, closed=True):
        o = C.c_void_p()
        rc = fb.lib.fb_lss_dlqr(h, pd(Q), pd(R), None, None, None, None, None, C.byref(o) if closed else None)
        assert not o.value or rc == 0          # a refusal leaves no handle
        if o.value:
            fb.lib.fb_destroy(o)
        return rc

    def refused(h, cause, call, name=b"fb_lss_dlqr"):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        rc = call()
        err = fb.lib.fb_last_error()
        assert rc != 0 and cause in err and name in err and launches(h) == 0, (cause, err)

    I3, I2 = np.eye(3), np.eye(2)
    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(ac._h, b"not a LinearizedSS handle", lambda: dlqr(ac._h, np.eye(20), np.eye(4)))
    ac.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 2, 3, n, 0, C.byref(h)) == 0
    refused(h, b"no model yet", lambda: dlqr(h, I3, I2))
    fb.lib.fb_destroy(h)
    A, B = rng.standard_normal((n, 3, 3)), rng.standard_normal((n, 3, 2))
    w = fb.LinearWorld(fb.design_model(A, B))
    refused(w._h, b"a discrete-time verb on a continuous model", lambda: dlqr(w._h, I3, I2))
    assert b"fb_lss_c2d" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError, match="fb_lss_c2d"):
        fb.dlqr(w, I3, I2)
    big = fb.LinearWorld(fb.design_model(rng.standard_normal((n, 17, 17)) - 6 * np.eye(17), rng.standard_normal((n, 17, 2))))
    sbig = fb.c2d(big, 0.02).world
    refused(sbig._h, b"nx = 17", lambda: dlqr(sbig._h, np.eye(17), I2))
    sbig.close()
    big.close()
    s = fb.c2d(w, 0.02).world
    Qu = np.eye(3); Qu[0, 1] = 1e-300
    refused(s._h, b"Q is not symmetric", lambda: dlqr(s._h, Qu, I2))
    Ru = np.eye(2); Ru[1, 0] = 0.5
    refused(s._h, b"R is not symmetric", lambda: dlqr(s._h, I3, Ru))
    refused(s._h, b"R is not positive definite", lambda: dlqr(s._h, I3, np.array([[1.0, 2.0], [2.0, 1.0]])))
    refused(s._h, b"Q and R are required", lambda: dlqr(s._h, None, I2))
    refused(s._h, b"Q and R are required", lambda: dlqr(s._h, I3, None))
    Qn = np.eye(3); Qn[1, 1] = np.inf
    refused(s._h, b"Q has a non-finite entry", lambda: dlqr(s._h, Qn, I2))
    with pytest.raises(fb.FlightBatchError, match="not positive definite"):
        fb.dlqr(s, np.ones(3), np.array([1.0, -1.0]))
    with pytest.raises(ValueError):
        fb.dlqr(s, np.eye(4), I2)
    # fb_lqr on the sampled handle: refused as before
    refused(s._h, b"a continuous-time verb on a sampled model", lambda: fb.lib.fb_lqr(s._h, None, None, None, None, None, None, None), b"fb_lqr")
    # valid calls: one stamp per kernel on the source's stream, with and without a closed world; all outputs NULL is a valid call
    for closed in (False, True):
        assert fb.lib.fb_timing_begin_per_launch(s._h, 8) == 0
        assert dlqr(s._h, I3, I2, closed=closed) == 0, fb.lib.fb_last_error()
        assert launches(s._h) == 1
    res = fb.dlqr(s, np.ones(3), np.ones(2))
    assert (res.iters > 0).all() and res.world is None          # (and the handle still designs)
    s.close()
    w.close()
