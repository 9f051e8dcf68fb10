"""fb_lqr (flightbatch.lqr): lqr(P, Q, R) for a batch of LinearizedSS models on the device, pinned by

  4. scipy's Schur solver on random systems of every group size, through the numpy restatement of the kernel's algorithm
     (tests/lqr_prototype.py; tests/test_lqr_host.py holds the prototype itself to scipy first);
  5. position independence and reproducibility, bit for bit, and the handle left as it was;
  6. the three systems without a stabilising solution, flagged in place among healthy neighbours;
  7. the reference's five stored gain tables, redesigned end to end on the device at the 28 nodes;
  8. the designed loop flown as a LinearWorld;
  9. the refusals of the C ABI on a live device.

The bound of 4 and 7: the device differs from the prototype in FMA contraction and <= 1-ulp division only, so its deviation from scipy may be
ten times the prototype's over the same systems, with the project's fp64 parity bound of 1e-11 as the floor."""
import ctypes as C
import functools

import numpy as np
import pytest

import lqr_prototype as proto
import reference_fixtures as rf

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-11, 10.0
NMAX = 130


@functools.lru_cache(maxsize=None)
def _reference(nx, nu):
    """the 130 systems of one shape with the prototype's and scipy's designs (computed once, read only)"""
    A, B, Q, R = proto.systems(nx, nu, NMAX)
    got = proto.lqr_batch(A, B, Q, R)
    Ks, Xs = proto.scipy_batch(A, B, Q, R)
    for a in (A, B, Q, R, Ks, Xs, *got.values()):
        a.setflags(write=False)
    return A, B, Q, R, got, Ks, Xs


def _world(fb, A, B, x0=None):
    return fb.LinearWorld(fb.design_model(A, B, x0=x0))


def _dev(got, want):
    return proto.rel_dev(got, want)


# ---- 4. every shape and batch edge against scipy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, NMAX])
@pytest.mark.parametrize("nx,nu", proto.SHAPES)
def test_random_systems_against_scipy(fb, nx, nu, n, capsys):
    A, B, Q, R, pr, Ks, Xs = _reference(nx, nu)
    w = _world(fb, A[:n], B[:n])
    Am, Bm = w.model()
    assert np.array_equal(Am, A[:n]) and np.array_equal(Bm, B[:n])
    res = fb.lqr(w, Q, R)
    w.close()
    assert res.K.shape == (n, nu, nx) and res.X.shape == (n, nx, nx) and res.resid.shape == res.iters.shape == res.status.shape == (n,)
    dK, dX = _dev(res.K, Ks[:n]), _dev(res.X, Xs[:n])
    pK, pX = _dev(pr["K"][:n], Ks[:n]), _dev(pr["X"][:n], Xs[:n])
    di = np.abs(res.iters.astype(int) - pr["iters"][:n]).max()
    with capsys.disabled():
        print(f"\n[fb_lqr vs scipy] ({nx:2d}, {nu}) x {n:3d}: K {dK:.2e} (prototype {pK:.2e})  X {dX:.2e} ({pX:.2e})  resid <= {res.resid.max():.2e} "
              f"({pr['resid'][:n].max():.2e})  iterations {res.iters.min()} - {res.iters.max()} (|device - prototype| <= {di})  "
              f"status {np.unique(res.status)}", end="")
    assert (res.status == 0).all()
    assert di <= 2
    assert dK <= max(MARGIN * pK, FLOOR) and dX <= max(MARGIN * pX, FLOOR)
    assert res.resid.max() <= max(MARGIN * pr["resid"][:n].max(), FLOOR)
    assert np.array_equal(res.X, res.X.transpose(0, 2, 1))


# ---- 5. position independence, reproducibility, and nothing written on the handle -------------------------------------------------------
def test_bitwise_independent_of_position_and_repeatable(fb):
    A, B, Q, R, *_ = _reference(11, 2)
    rng = np.random.default_rng(4)
    x0 = rng.standard_normal((NMAX, 11))
    w = _world(fb, A, B, x0=x0)
    w.u = rng.standard_normal((2, NMAX))
    w.step(7, dt=1e-3)
    w.sync()
    before = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model())
    first = fb.lqr(w, Q, R)
    again = fb.lqr(w, Q, R)
    after = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model())
    w.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[2] == pytest.approx(7e-3)
    assert (first.status == 0).all()
    same = lambda p, q, sel=slice(None): all(np.array_equal(getattr(p, k)[sel], getattr(q, k), equal_nan=True) for k in ("K", "X", "iters", "resid", "status"))
    assert same(first, again)
    wr = _world(fb, A[::-1], B[::-1])
    assert same(first, fb.lqr(wr, Q, R), slice(None, None, -1))
    wr.close()
    pick = np.array([129, 0, 64, 63, 17, 1, 100])
    ws = _world(fb, A[pick], B[pick])
    assert same(first, fb.lqr(ws, Q, R), pick)
    ws.close()


# ---- 6. failure lanes ----------------------------------------------------------------------------------------------------------------------
def test_systems_without_a_solution_are_flagged_in_place(fb):
    """66 (3, 1) systems, 5, 64 and 65 replaced by the three systems without a stabilising solution (the 2-state ones with a stable third
    state nothing couples to). Q and R are the batch's, so one pair has to serve all three: Q = diag(0, 0, 1), R = 1, the third system's own.
    The causes do not depend on that choice: the first system's unstable mode is uncontrollable whatever it is weighted with (W11 = 1 there:
    I - W11 is exactly singular), the second's Hamiltonian has a zero row pair (a = b = 0 in its first state), the third's uncontrollable,
    unweighted oscillator keeps a pair of eigenvalues of the Hamiltonian on the imaginary axis. (A weight on that oscillator would leave the
    eigenvalues where they are, but the iteration then grows a block without bound and its outcome depends on rounding.) The inputs are
    fixed and nothing is retried: the iteration bound is what ends the third."""
    A, B, _, _ = proto.systems(3, 1, 66)
    A, B = A.copy(), B.copy()
    Q, R = np.diag([0.0, 0.0, 1.0]), np.eye(1)
    where, want = (5, 64, 65), []
    for i, (a, b, q, _, st) in zip(where, proto.failure_systems()):
        A[i], B[i], _ = proto.embed3(a, b, q)
        want.append(st)
        assert proto.lqr(A[i], B[i], Q, R)["status"] == st
    w = _world(fb, A, B)
    K, X = np.empty(3 * 66), np.empty(9 * 66)
    resid, iters, status = np.empty(66), np.empty(66, dtype=np.int32), np.empty(66, dtype=np.int32)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = fb.lib.fb_lqr(w._h, pd(np.asfortranarray(Q).reshape(-1, order="F")), pd(R.reshape(-1)), pd(K), pd(X), pd(resid), pi(iters), pi(status))
    assert rc == 0, fb.lib.fb_last_error()
    res = fb.lqr(w, Q, R)
    w.close()
    assert np.array_equal(res.status, status) and np.array_equal(res.K.transpose(2, 1, 0).reshape(-1), K, equal_nan=True)
    expect = np.zeros(66, dtype=np.int32)
    expect[list(where)] = want
    assert np.array_equal(res.status, expect), res.status
    assert res.iters[65] == 50
    ok = expect == 0
    assert np.isnan(res.K[~ok]).all() and np.isnan(res.X[~ok]).all()
    assert np.isfinite(res.K[ok]).all() and np.isfinite(res.X[ok]).all() and np.isfinite(res.resid[ok]).all()
    wh = _world(fb, A[ok], B[ok])
    healthy = fb.lqr(wh, Q, R)
    wh.close()
    assert (healthy.status == 0).all()
    for k in ("K", "X", "iters", "resid"):
        assert np.array_equal(getattr(res, k)[ok], getattr(healthy, k))


# ---- 7. the reference's stored gain tables, on the device from trim to gain ---------------------------------------------------------------
def _assemble(rl, name, Ap, Bp):
    """the (augmented) A, B, Q, R of one design at one node as reference_lqr.design builds them, and what K_fwd needs"""
    xl, ul, zl, qx, qi, r, fwd = rl.DESIGNS[name]
    A, B = rl._sub(Ap, Bp, xl, ul)
    Cz, Dz = rl._z_rows(xl, ul, zl)
    nx, nz = len(xl), len(zl)
    q = [float(qx.get(k, 0.0)) for k in xl]
    if qi is not None:
        A_aug = np.block([[A, np.zeros((nx, nz))], [Cz, np.zeros((nz, nz))]])
        B_aug = np.vstack([B, Dz])
        q = q + [float(v) for v in qi]
    else:
        A_aug, B_aug = A, B
    return A_aug, B_aug, np.array(q), np.array(r, dtype=np.float64), (A, B, Cz, Dz, nx, nz, fwd)


def test_the_references_gain_tables_designed_on_the_device(fb, capsys):
    import reference_lqr as rl
    EAS, h, flaps = rf.design_nodes()
    w = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme="onesided2")
    w.close()
    assert lss.success.all() and (lss.status == 0).all()
    iy = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    models = [rl.design_model(lss.A[k], lss.B[k], lss.C[k][iy]) for k in range(28)]
    for name in rl.DESIGNS:
        parts = [_assemble(rl, name, *models[k]) for k in range(28)]
        A = np.array([p[0] for p in parts]); B = np.array([p[1] for p in parts])
        q, r = parts[0][2], parts[0][3]
        lw = _world(fb, A, B)
        res = fb.lqr(lw, q, r)
        lw.close()
        assert (res.status == 0).all(), (name, res.status)
        st = rf.stored(name)
        dev = {"K_fbk": 0.0, "K_fwd": 0.0, "K_int": 0.0}
        d_scipy = p_scipy = 0.0
        for k in range(28):
            A0, B0, Cz, Dz, nx, nz, fwd = parts[k][4]
            Kk = res.K[k]
            got = {"K_fbk": Kk[:, :nx], "K_int": Kk[:, nx:] if Kk.shape[1] > nx else np.zeros((Kk.shape[0], nz)),
                   "K_fwd": np.eye(nz) if fwd == "identity" else rl._k_fwd(A0, B0, Cz, Dz, Kk[:, :nx])}
            for m in dev:
                want = st[m][..., k]
                scale = np.abs(want).max() if np.abs(want).max() > 0 else 1.0
                dev[m] = max(dev[m], np.abs(got[m] - want).max() / scale)
            # the same A, B through scipy (reference_lqr.design) and through the prototype
            Kd, _, Kid = rl.design(name, *models[k])
            Ks = np.hstack([Kd, Kid]) if Kk.shape[1] > nx else Kd
            Kp = proto.lqr(A[k], B[k], np.diag(q), np.diag(r))["K"]
            d_scipy = max(d_scipy, np.abs(Kk - Ks).max() / np.abs(Ks).max())
            p_scipy = max(p_scipy, np.abs(Kp - Ks).max() / np.abs(Ks).max())
        with capsys.disabled():
            print(f"\n[fb_lqr {name:10s}] nx {A.shape[1]:2d}: vs the stored tables K_fbk {dev['K_fbk']:.2e}  K_fwd {dev['K_fwd']:.2e}  K_int {dev['K_int']:.2e}; "
                  f"vs scipy on the same A, B {d_scipy:.2e} (prototype {p_scipy:.2e}); iterations {res.iters.min()} - {res.iters.max()}, "
                  f"resid <= {res.resid.max():.2e}", end="")
        assert max(dev.values()) <= 5e-6, (name, dev)
        assert d_scipy <= max(MARGIN * p_scipy, FLOOR), (name, d_scipy, p_scipy)


# ---- 8. design, then fly ---------------------------------------------------------------------------------------------------------------------
def test_the_designed_loop_returns_to_its_design_point(fb, capsys):
    A, B, Q, R, *_ = _reference(8, 2)
    rng = np.random.default_rng(8)
    x0 = rng.standard_normal((NMAX, 8))
    lss = fb.design_model(A, B, x0=x0)
    w = fb.LinearWorld(lss)
    K = fb.lqr(w, Q, R).K
    w.close()
    cl = fb.closed_loop(lss, K)
    dx0 = rng.standard_normal((NMAX, 8))
    lam = np.array([np.linalg.eigvals(cl.A[i]).real.max() for i in range(NMAX)])
    assert (lam < 0).all()
    dt = 0.05 / np.abs(cl.A).sum(axis=2).max()
    nsteps = int(np.ceil(20.0 / np.abs(lam).min() / dt))
    scale = np.linalg.norm(dx0, axis=1)
    ends = {}
    for tag, model in (("closed", cl), ("open", lss)):
        lw = fb.LinearWorld(model)
        lw.set_state((x0 + dx0).T)
        lw.step(nsteps, dt=dt, steps_per_launch=1000)
        lw.sync()
        ends[tag] = np.abs(lw.x.T - x0).max(axis=1) / scale
        lw.close()
    unstable = np.array([np.linalg.eigvals(A[i]).real.max() for i in range(NMAX)]) > 0.05
    with capsys.disabled():
        print(f"\n[fb_lqr, flown] 130 (8, 2) loops, {nsteps} steps of {dt:.3e}: max |x - x0| / |dx(0)| closed {ends['closed'].max():.2e}; "
              f"open loop, {unstable.sum()} unstable plants: min over them {np.nanmin(ends['open'][unstable]):.2e}", end="")
    assert ends["closed"].max() <= 1e-6
    assert unstable.any() and not (ends["open"][unstable] <= 1e-6).any()


# ---- 9. refusals on a live device ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    rng = np.random.default_rng(9)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = lambda n, nx, nu: (pd(np.empty(nu * nx * n)), pd(np.empty(nx * nx * n)), pd(np.empty(n)), None, None)

    def refused(h, Q, R, nx, nu, n, msg):
        t0 = fb.lib.fb_time(h)
        st0 = np.empty(n, dtype=np.int32); st1 = np.empty(n, dtype=np.int32)
        assert fb.lib.fb_status(h, st0.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        rc = fb.lib.fb_lqr(h, pd(Q) if Q is not None else None, pd(R) if R is not None else None, *out(n, nx, nu))
        err = fb.lib.fb_last_error()
        assert rc != 0 and msg in err, err
        assert fb.lib.fb_status(h, st1.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        assert fb.lib.fb_time(h) == t0 and np.array_equal(st0, st1)

    n = 5
    big = _world(fb, rng.standard_normal((n, 17, 17)) - 6 * np.eye(17), rng.standard_normal((n, 17, 2)))
    big.step(3, dt=1e-3)
    refused(big._h, np.eye(17).reshape(-1), np.eye(2).reshape(-1), 17, 2, n, b"nx = 17")
    big.close()
    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(ac._h, np.eye(20).reshape(-1), np.eye(4).reshape(-1), 20, 4, n, b"not a LinearizedSS handle")
    ac.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 3, n, 0, C.byref(h)) == 0
    refused(h, np.eye(3).reshape(-1), np.eye(1).reshape(-1), 3, 1, n, b"no model yet")
    assert fb.lib.fb_lss_get_model(h, None, None) != 0 and b"no model yet" in fb.lib.fb_last_error()
    fb.lib.fb_destroy(h)
    w = _world(fb, rng.standard_normal((n, 3, 3)), rng.standard_normal((n, 3, 2)))
    w.step(3, dt=1e-3)
    Qu = np.eye(3); Qu[0, 1] = 1e-300
    refused(w._h, Qu.reshape(-1), np.eye(2).reshape(-1), 3, 2, n, b"Q is not symmetric")
    Ru = np.eye(2); Ru[1, 0] = 0.5
    refused(w._h, np.eye(3).reshape(-1), Ru.reshape(-1), 3, 2, n, b"R is not symmetric")
    refused(w._h, np.eye(3).reshape(-1), np.array([[1.0, 2.0], [2.0, 1.0]]).reshape(-1), 3, 2, n, b"R is not positive definite")
    refused(w._h, None, np.eye(2).reshape(-1), 3, 2, n, b"Q and R are required")
    with pytest.raises(fb.FlightBatchError, match="not positive definite"):
        fb.lqr(w, np.ones(3), np.array([1.0, -1.0]))
    with pytest.raises(ValueError):
        fb.lqr(w, np.eye(4), np.eye(2))
    assert (fb.lqr(w, np.ones(3), np.ones(2)).iters > 0).all()   # (and the handle still designs)
    w.close()
