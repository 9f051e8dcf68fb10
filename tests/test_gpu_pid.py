"""fb_lss_freqresp and fb_pid_metrics (flightbatch.pidopt): the metrics of the reference's optimize_PID for a batch of linear models and PID
candidates on the device, and the pattern search on top of them, pinned by

  5. np.linalg.solve on random plants of every group size and both of its edges;
  6. exact discretisation (scipy's expm) and np.linalg.solve on random loops that are stable by construction, d = 0 and d > 0;
  7. position independence and reproducibility, bit for bit, and the handle left as it was;
  8. a diverging and a singular pair flagged in place among healthy ones;
  9. the reference's stored q2e gains at the 28 design nodes, from the device's own trim, linearisation and te2te design;
 10. optimize_pid on those 28 plants against the stored gains' cost;
 11. the refusals of the C ABI on a live device.

The bound of 5, 6 and 9 is the LQR tests' rule: the device differs from the numpy restatement of its algorithm (tests/pid_prototype.py; held
to the exact side on the CPU by tests/test_pid_host.py) in FMA contraction, summation order and <= 1-ulp division only, so its deviation
from the exact side may be ten times the prototype's over the same pairs, with the project's fp64 parity bound of 1e-11 as the floor. A
deviation is |got - exact| / |exact| per metric, the worst over the pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import pid_prototype as proto
import reference_fixtures as rf
from support import pd

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-11, 10.0
NAMES = ("Ms", "ie", "ef", "iu", "up")
N_REF, M_REF = 9, 5
T_SIM, DT = 2.0, 1e-3
IU, IY = 1, 2
pi32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def _world(fb, A, b, c, d, seed=5):
    """the plants as channel (IU, IY) of two-input, three-output models whose other channels, and whose xdot0, x0, u0, y0, are random numbers
    (they play no part)"""
    n, nx = b.shape
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, nx, 2)); B[:, :, IU] = b
    Cm = rng.standard_normal((n, 3, nx)); Cm[:, IY, :] = c
    D = rng.standard_normal((n, 3, 2)); D[:, IY, IU] = d
    lss = fb.LinearizedSS(xdot0=rng.standard_normal((n, nx)), x0=rng.standard_normal((n, nx)), u0=rng.standard_normal((n, 2)),
                          y0=rng.standard_normal((n, 3)), A=A, B=B, C=Cm, D=D, x_labels=tuple(f"x{k}" for k in range(nx)),
                          u_labels=("other", "u"), y_labels=("y0", "y1", "y"))
    return fb.LinearWorld(lss)


@functools.lru_cache(maxsize=None)
def _freq_reference(nx):
    A, b, c, d = proto.plants(nx, N_REF)
    pw = np.array([proto.freqresp(A[i], b[i], c[i], d[i], proto.W7) for i in range(N_REF)])
    pe = np.array([proto.freqresp_exact(A[i], b[i], c[i], d[i], proto.W7) for i in range(N_REF)])
    for a in (A, b, c, d, pw, pe):
        a.setflags(write=False)
    return A, b, c, d, pw, pe


@functools.lru_cache(maxsize=None)
def _metrics_reference(nx):
    """the 9 x 5 pairs of one nx with the prototype's and the exact side's metrics [9, 5, 5] (computed once, read only)"""
    A, b, c, d = proto.plants(nx, N_REF)
    P = proto.points(N_REF, M_REF)
    rep = lambda a: np.repeat(a, M_REF, axis=0)
    args = (rep(A), rep(b), rep(c), rep(d), P.reshape(-1, 4), proto.W7, T_SIM, DT)
    got, _, st = proto.metrics(*args)
    want, _, ste = proto.metrics(*args, side="exact")
    assert (st == 0).all() and (ste == 0).all()
    out = (A, b, c, d, P, got.reshape(N_REF, M_REF, 5), want.reshape(N_REF, M_REF, 5))
    for a in out:
        a.setflags(write=False)
    return out


def _hold(tag, got, want, pro, capsys):
    """the rule of the module docstring per metric; prints the device's and the prototype's deviation"""
    dd, dp = proto.rel_dev(got, want), proto.rel_dev(pro, want)
    with capsys.disabled():
        print(f"\n[{tag}] " + "  ".join(f"{k} {a:.2e} ({b:.2e})" for k, a, b in zip(NAMES, dd, dp)), end="")
    for k, a, b in zip(NAMES, dd, dp):
        assert a <= max(MARGIN * b, FLOOR), (tag, k, a, b)


# ---- 5. P(jw) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("nx", [1, 8, 9, 16, 17, 28])
def test_freqresp_against_linalg_solve(fb, nx, n, capsys):
    A, b, c, d, pw, pe = _freq_reference(nx)
    w = _world(fb, A[:n], b[:n], c[:n], d[:n])
    got = fb.freqresp(w, u="u", y="y", w=proto.W7)
    w.close()
    assert got.shape == (n, 7) and np.isfinite(got).all()
    dev = float((np.abs(got - pe[:n]) / np.abs(pe[:n])).max())
    dpr = float((np.abs(pw[:n] - pe[:n]) / np.abs(pe[:n])).max())
    with capsys.disabled():
        print(f"\n[fb_lss_freqresp vs solve] nx {nx:2d} x {n}: {dev:.2e} (prototype {dpr:.2e})", end="")
    assert dev <= max(MARGIN * dpr, FLOOR)


# ---- 6. the metrics ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("nx", [1, 4, 5, 12, 13, 28])
def test_metrics_against_the_exact_side(fb, nx, n, m, capsys):
    A, b, c, d, P, pro, exact = _metrics_reference(nx)
    weights = None if m == 1 else proto.Q2E_WEIGHTS
    w = _world(fb, A[:n], b[:n], c[:n], d[:n])
    res = fb.pid_metrics(w, P[:n, :m], u=IU, y=IY, settings=fb.Settings(t_sim=T_SIM, dt=DT, w=proto.W7), weights=weights)
    w.close()
    assert res.metrics.shape == (n, m, 5) and res.cost.shape == res.status.shape == (n, m)
    assert (res.status == 0).all()
    assert n == 1 or ((d[:n] == 0).any() and (d[:n] > 0).any())
    _hold(f"fb_pid_metrics vs exact, nx {nx:2d}, {n} x {m}", res.metrics, exact[:n, :m], pro[:n, :m], capsys)
    wt = np.ones(5, dtype=np.longdouble) if weights is None else np.array(weights, dtype=np.longdouble)
    want = np.array((res.metrics.astype(np.longdouble) * wt).sum(axis=2) / wt.sum(), dtype=np.float64)
    assert (np.abs(res.cost - want) <= 1e-15 * want).all(), np.abs(res.cost / want - 1).max()


# ---- 7. bits ---------------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_independent_of_position_and_slot_and_repeatable(fb):
    A, b, c, d, P, _, _ = _metrics_reference(12)
    st = fb.Settings(t_sim=T_SIM, dt=DT, w=proto.W7)
    run = lambda world, pts: fb.pid_metrics(world, pts, u=IU, y=IY, settings=st, weights=proto.Q2E_WEIGHTS)
    same = lambda p, q, sel=slice(None): all(np.array_equal(getattr(p, k)[sel], getattr(q, k)) for k in ("metrics", "cost", "status"))
    w = _world(fb, A, b, c, d)
    rng = np.random.default_rng(7)
    w.set_state(rng.standard_normal((12, N_REF)))
    w.u = rng.standard_normal((2, N_REF))
    w.step(7, dt=1e-3)
    w.sync()
    before = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model())
    first = run(w, P)
    again = run(w, P)
    f1 = fb.freqresp(w, u=IU, y=IY, w=proto.W7)
    after = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model())
    for p, q in zip(before, after):
        assert np.array_equal(p, q)
    assert before[2] == pytest.approx(7e-3) and (first.status == 0).all()
    assert same(first, again) and np.array_equal(f1, fb.freqresp(w, u=IU, y=IY, w=proto.W7))
    # a candidate's slot: the candidates permuted, and each one alone
    perm = np.array([3, 0, 4, 2, 1])
    shuffled = run(w, P[:, perm])
    assert all(np.array_equal(getattr(first, k)[:, perm], getattr(shuffled, k)) for k in ("metrics", "cost", "status"))
    alone = run(w, P[:, 2:3])
    assert all(np.array_equal(getattr(first, k)[:, 2:3], getattr(alone, k)) for k in ("metrics", "cost", "status"))
    w.close()
    # a system's position: the batch reversed, and a scattered subset
    for pick in (np.arange(N_REF)[::-1], np.array([8, 0, 5, 3])):
        ws = _world(fb, A[pick], b[pick], c[pick], d[pick], seed=6)   # (other channels than the full batch's: they play no part)
        assert np.array_equal(ws.model()[0], before[4][pick])
        assert same(first, run(ws, P[pick]), pick)
        assert np.array_equal(f1[pick], fb.freqresp(ws, u=IU, y=IY, w=proto.W7))
        ws.close()



# ---- 8. failure lanes ------------------------------------------------------------------------------------------------------------------------------
def test_diverging_and_singular_pairs_are_flagged_in_place(fb):
    """Seven one-state plants, three candidates each. System 2 is 1 / (s - 20): with p = (1, 0, 0, 0.01) in slot 1 its loop pole is +19 and
    e^38 > 1e12 inside t_sim = 2 (its other candidates have k_p = 30: pole -10). System 5 is 1 / (s + 1) - 0.5: with p = (2, 0, 0, 0.01) in
    slot 0, d Dc = -1 exactly (its other candidates, (0.5, 0.5, 0, 0.01), close a stable loop: 0.75 s^2 + s + 0.25). The inputs are fixed and
    nothing is retried: the overflow is arithmetic, by design of the input."""
    n, m = 7, 3
    A, b, c, d = (a.copy() for a in proto.plants(1, n))
    P = proto.points(n, m).copy()
    A[2], b[2], c[2], d[2] = 20.0, 1.0, 1.0, 0.0
    P[2] = np.array([30.0, 0.0, 0.0, 0.01]); P[2, 1] = np.array([1.0, 0.0, 0.0, 0.01])
    A[5], b[5], c[5], d[5] = -1.0, 1.0, 1.0, -0.5
    P[5] = np.array([0.5, 0.5, 0.0, 0.01]); P[5, 0] = np.array([2.0, 0.0, 0.0, 0.01])
    st = fb.Settings(t_sim=T_SIM, dt=DT, w=proto.W7)
    rep = lambda a: np.repeat(a, m, axis=0)
    pm, pc, ps = proto.metrics(rep(A), rep(b), rep(c), rep(d), P.reshape(-1, 4), proto.W7, T_SIM, DT)
    expect = np.zeros((n, m), dtype=np.int32); expect[2, 1] = fb.pidopt.DIVERGED; expect[5, 0] = fb.pidopt.SINGULAR
    assert np.array_equal(ps.reshape(n, m), expect)
    w = _world(fb, A, b, c, d)
    res = fb.pid_metrics(w, P, u=IU, y=IY, settings=st)
    healthy = P.copy(); healthy[2, 1] = P[2, 0]; healthy[5, 0] = P[5, 1]
    ref = fb.pid_metrics(w, healthy, u=IU, y=IY, settings=st)
    w.close()
    assert np.array_equal(res.status, expect), res.status
    assert (ref.status == 0).all() and np.isfinite(ref.metrics).all() and np.isfinite(ref.cost).all()
    dv = res.metrics[2, 1]
    assert np.isinf(dv[1:]).all() and (dv[1:] > 0).all() and np.isfinite(dv[0]) and res.cost[2, 1] == np.inf
    assert abs(dv[0] - pm.reshape(n, m, 5)[2, 1, 0]) <= 1e-12 * dv[0]          # Ms is still the grid's
    assert np.isnan(res.metrics[5, 0]).all() and res.cost[5, 0] == np.inf
    ok = expect == 0
    assert np.array_equal(res.metrics[ok], ref.metrics[ok]) and np.array_equal(res.cost[ok], ref.cost[ok])


# ---- 9, 10. the reference's q2e loop, on the device from trim to metrics -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _q2e_on_the_device(fb):
    """A [28, 9, 9], b, c [28, 9], d [28] of P_q2e_opt (c172x_design.jl:222-227): linearize at the 28 nodes as tests/test_gpu_lqr.py does, te2te
    by fb.lqr, K_fwd and the loop closed on the host"""
    import reference_lqr as rl
    EAS, h, flaps = rf.design_nodes()
    w = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme="onesided2")
    w.close()
    assert lss.success.all() and (lss.status == 0).all()
    iy = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    xl, ul, zl, qx, _, r, _ = rl.DESIGNS["te2te"]
    red = [rl._sub(*rl.design_model(lss.A[k], lss.B[k], lss.C[k][iy]), xl, ul) for k in range(28)]
    Ar, Br = np.array([p[0] for p in red]), np.array([p[1] for p in red])
    lw = fb.LinearWorld(fb.design_model(Ar, Br))
    res = fb.lqr(lw, [float(qx.get(k, 0.0)) for k in xl], np.array(r, dtype=np.float64))
    lw.close()
    assert (res.status == 0).all()
    Cz, Dz = rl._z_rows(xl, ul, zl)
    parts = [proto.q2e_plant(Ar[k], Br[k], res.K[k], rl._k_fwd(Ar[k], Br[k], Cz, Dz, res.K[k]), iq=xl.index("q"), i_ele=ul.index("elevator_cmd"))
             for k in range(28)]
    out = tuple(np.array([p[j] for p in parts]) for j in range(4))
    for a in out:
        a.setflags(write=False)
    return out


def test_the_references_q2e_table_on_the_device(fb, capsys):
    A, b, c, d = _q2e_on_the_device(fb)
    P = proto.q2e_stored()
    w = fb.LinearWorld(proto.model(fb, A, b, c, d))
    assert w.nx == 9
    res = fb.pid_metrics(w, P[:, None, :], settings=fb.Settings(t_sim=proto.Q2E_T_SIM, dt=1e-3, w=proto.Q2E_GRID), weights=proto.Q2E_WEIGHTS)
    w.close()
    got = res.metrics[:, 0]
    with capsys.disabled():
        print(f"\n[q2e, stored gains, on the device] worst over 28 nodes: Ms {got[:, 0].max():.4f}  ie {got[:, 1].max():.4f}  ef {got[:, 2].max():.4f}  "
              f"iu {got[:, 3].max():.4f}  up {got[:, 4].max():.3f}; cost {res.cost.min():.4f} .. {res.cost.max():.4f}", end="")
    assert (res.status == 0).all()
    assert fb.check_results(res.metrics[:, 0], fb.Metrics(*proto.Q2E_THRESHOLDS)).all()
    args = (A, b, c, d, P, proto.Q2E_GRID, proto.Q2E_T_SIM, 1e-3)
    pro, _, _ = proto.metrics(*args, weights=proto.Q2E_WEIGHTS)
    exact, _, _ = proto.metrics(*args, weights=proto.Q2E_WEIGHTS, side="exact")
    _hold("fb_pid_metrics vs exact, q2e, 28 nodes", got, exact, pro, capsys)


def test_optimize_pid_on_the_28_q2e_plants(fb, capsys):
    A, b, c, d = _q2e_on_the_device(fb)
    stored = proto.q2e_stored()
    S, P = fb.Settings, fb.PIDData
    st = S(t_sim=proto.Q2E_T_SIM, lower_bounds=P(*proto.Q2E_LOWER), upper_bounds=P(*proto.Q2E_UPPER), dt=2e-3, w=proto.Q2E_GRID)
    w = fb.LinearWorld(proto.model(fb, A, b, c, d))
    ref = fb.pid_metrics(w, stored[:, None, :], settings=st, weights=fb.Metrics(*proto.Q2E_WEIGHTS))
    opt = fb.optimize_pid(w, data_0=P(*proto.Q2E_DATA_0), settings=st, weights=fb.Metrics(*proto.Q2E_WEIGHTS))
    w.close()
    with capsys.disabled():
        print("\n[optimize_pid, q2e] node | stored k_p k_i k_d | found k_p k_i k_d | cost stored, found, ratio | iterations, evaluations")
        for k in range(28):
            print(f"  {k:2d} | {stored[k, 0]:7.4f} {stored[k, 1]:8.4f} {stored[k, 2]:7.4f} | {opt.data[k, 0]:7.4f} {opt.data[k, 1]:8.4f} {opt.data[k, 2]:7.4f} | "
                  f"{ref.cost[k, 0]:.6f} {opt.cost[k]:.6f} {opt.cost[k] / ref.cost[k, 0]:.5f} | {opt.iters[k]:2d} {opt.evals[k]:4d}")
        print(f"  ratio {np.min(opt.cost / ref.cost[:, 0]):.5f} .. {np.max(opt.cost / ref.cost[:, 0]):.5f}; Ms <= {opt.metrics[:, 0].max():.4f}  "
              f"ie <= {opt.metrics[:, 1].max():.4f}  ef <= {opt.metrics[:, 2].max():.4f}; iterations {opt.iters.min()} - {opt.iters.max()}", end="")
    assert (ref.status == 0).all() and (opt.status == 0).all()
    assert (opt.iters <= 80).all()
    assert (opt.cost <= 1.01 * ref.cost[:, 0]).all()
    assert fb.check_results(opt, fb.Metrics(*proto.Q2E_THRESHOLDS)).all()
    assert (opt.data[:, 3] == 0.01).all() and (opt.data >= np.array(proto.Q2E_LOWER)).all() and (opt.data <= np.array(proto.Q2E_UPPER)).all()


# ---- 11. refusals on a live device ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n, m, nw = 4, 2, 3
    grid = np.array([0.5, 1.0, 2.0])
    pts = np.tile(np.array([1.0, 0.5, 0.0, 0.02])[:, None, None], (1, m, n)).copy()        # [4 x m x N]
    ones = np.ones(5)

    def call(h, iu=0, iy=0, w=grid, nw=nw, t_sim=1.0, dt=1e-2, weights=ones, pid=pts, m=m, metrics=True, cost=True, status=True):
        met, co, st = np.empty(5 * m * n if m > 0 else 1), np.empty(max(m, 1) * n), np.empty(max(m, 1) * n, dtype=np.int32)
        return fb.lib.fb_pid_metrics(h, iu, iy, pd(w) if w is not None else None, nw, t_sim, dt, pd(weights) if weights is not None else None,
                                     pd(pid) if pid is not None else None, m, pd(met) if metrics else None, pd(co) if cost else None,
                                     pi32(st) if status else None)

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def refused(h, msg, freq=False, **kw):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        if freq:
            re, im = np.empty(1024 * n), np.empty(1024 * n)
            wv = kw.get("w", grid)
            rc = fb.lib.fb_lss_freqresp(h, kw.get("iu", 0), kw.get("iy", 0), pd(wv) if wv is not None else None, kw.get("nw", nw), pd(re), pd(im))
        else:
            rc = call(h, **kw)
        err = fb.lib.fb_last_error()
        assert rc != 0 and msg in err, err
        assert launches(h) == 0

    A, b, c, d = proto.plants(3, n)
    w = fb.LinearWorld(proto.model(fb, A, b, c, d))
    h = w._h
    bad_tau = pts.copy(); bad_tau[3, 1, 2] = 0.0
    nan_tau = pts.copy(); nan_tau[3, 0, 0] = np.nan
    for kw, msg in ((dict(iu=1), b"iu = 1"), (dict(iu=-1), b"iu = -1"), (dict(iy=1), b"iy = 1"), (dict(w=None), b"grid w is required"),
                    (dict(nw=0), b"nw = 0"), (dict(w=np.ones(1025), nw=1025), b"nw = 1025"), (dict(w=np.array([1.0, 0.0, 2.0])), b"w[1]"),
                    (dict(w=np.array([1.0, 2.0, np.inf])), b"w[2]"), (dict(w=np.array([-1.0, 2.0, 3.0])), b"w[0]")):
        refused(h, msg, **kw)
        refused(h, msg, freq=True, **kw)
    for kw, msg in ((dict(m=0), b"m = 0"), (dict(m=65), b"m = 65"), (dict(dt=0.0), b"dt = 0"), (dict(dt=-1e-3), b"dt = -0.001"),
                    (dict(dt=np.nan), b"dt = nan"), (dict(t_sim=5e-3), b"at least dt"), (dict(t_sim=np.inf), b"t_sim = inf"),
                    (dict(t_sim=10.0, dt=1e-5), b"at most 200000"), (dict(pid=bad_tau), b"tau_f = 0 at system 2, candidate 1"),
                    (dict(pid=nan_tau), b"tau_f = nan at system 0, candidate 0"), (dict(weights=np.array([1.0, 1.0, -1.0, 1.0, 1.0])), b"weights[2]"),
                    (dict(weights=np.zeros(5)), b"weights sum to zero"), (dict(pid=None), b"are required"), (dict(cost=False), b"are required"),
                    (dict(status=False), b"are required")):
        refused(h, msg, **kw)
    # and the handle still evaluates: two stamped launches (the frequency response, then the metrics), null weights = ones, null metrics
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert call(h, weights=None, metrics=False) == 0, fb.lib.fb_last_error()
    assert launches(h) == 2
    w.close()
    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(ac._h, b"not a LinearizedSS handle")
    refused(ac._h, b"not a LinearizedSS handle", freq=True)
    ac.close()
    hh = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 1, n, 0, C.byref(hh)) == 0
    refused(hh, b"no model yet")
    refused(hh, b"no model yet", freq=True)
    fb.lib.fb_destroy(hh)
    A, b, c, d = proto.plants(29, n)
    big = fb.LinearWorld(proto.model(fb, A, b, c, d))
    refused(big._h, b"nx = 29")
    refused(big._h, b"nx = 29", freq=True)
    big.close()
