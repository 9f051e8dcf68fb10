"""PID loop design on the device, host side (no GPU compute; docs/design/linearize.md, "PID loop design on the device"):

  1. the numpy restatement of the kernels' algorithm (tests/pid_prototype.py) against exact discretisation and np.linalg.solve on the random
     plants the GPU tests use — the deviations printed here are what the GPU bound multiplies;
  2. the reference's stored q2e gains on the oracle's Jacobian at the 28 design nodes meet the reference's acceptance thresholds
     (FA design/c172/c172x_design.jl:222-241);
  3. the pattern search of flightbatch.pidopt at node 13 from the reference's data_0, bounds and weights ends as good as the stored gains;
  4. the refusals of flightbatch.pidopt that need no device.

Bounds. RK4 against the exact map: the global error of a mode lambda is (|lambda| dt)^4 / 120 per unit of |lambda| t, and only while the mode
is alive (a few time constants); the fastest modes of the random loops are the derivative filter's, |lambda| <= 1 / 0.02 + Dc |c b| <= 65 at
dt = 1e-3, so (0.065)^4 / 120 * 3 = 4.5e-7: asserted at 1e-6 on every metric. P(jw) by elimination with pivoting against LAPACK's: both are
backward stable, the systems' condition numbers are below 1e3 (|A| <= 10, w >= 0.1, spectral abscissa <= -0.5): asserted at 1e-12.
The one-map form of RK4 (pid_prototype.rk4_map_metrics, what test 3 searches on) rounds Phi once and applies it N times: a relative
perturbation of the loop's matrix by eps / dt = 1e-13, which a metric that is a difference from 1 (ef, down to 1e-3 here) sees as 1e-10
relative: asserted at 1e-9 against the stage form."""
import functools

import numpy as np
import pytest

import pid_prototype as proto
import reference_fixtures as rf
import reference_lqr as rl

pytest.importorskip("scipy.linalg")
NX = (1, 4, 5, 8, 9, 12, 13, 16, 17, 28)


def test_new_symbols_and_names(fb):
    assert (fb.K["FB_PID_DIVERGED"], fb.K["FB_PID_SINGULAR"], fb.K["FB_PID_NX_MAX"]) == (proto.DIVERGED, proto.SINGULAR, 28)
    assert "fb_lss_freqresp" in fb.EXPORTED and "fb_pid_metrics" in fb.EXPORTED
    assert len(fb.lib.fb_lss_freqresp.argtypes) == 7 and len(fb.lib.fb_pid_metrics.argtypes) == 13
    for name in ("PIDData", "Metrics", "Settings", "build_pid", "freqresp", "pid_metrics", "optimize_pid", "check_results"):
        assert hasattr(fb, name), name
    assert fb.lib.fb_lss_freqresp(None, 0, 0, None, 0, None, None) != 0 and b"null handle" in fb.lib.fb_last_error()
    assert fb.lib.fb_pid_metrics(None, 0, 0, None, 0, 1.0, 0.1, None, None, 1, None, None, None) != 0 and b"null handle" in fb.lib.fb_last_error()


def test_reference_field_names_defaults_and_aliases(fb):
    p = fb.PIDData()
    assert (p.k_p, p.k_i, p.k_d, p.τ_f, p.tau_f) == (1.0, 0.0, 0.1, 0.01, 0.01)                  # FP/control.jl:776-781
    assert np.array_equal(np.asarray(fb.PIDData(k_p=2, tau_f=0.5)), [2.0, 0.0, 0.1, 0.5])
    m = fb.Metrics(**{"Ms": 1.6, "∫e": 0.3, "ef": 0.04, "∫u": np.inf, "up": np.inf})               # c172x_design.jl:239
    assert (m.Ms, m.ie, m["∫e"], m.ef, m.iu, m["∫u"], m.up) == (1.6, 0.3, 0.3, 0.04, np.inf, np.inf, np.inf)
    assert np.array_equal(np.asarray(fb.Metrics(np.ones(5))), np.ones(5))
    with pytest.raises(TypeError):
        fb.Metrics(Ms=1.0)
    s = fb.Settings()                                                                             # pidopt.jl:16-22
    assert (s.t_sim, s.maxeval) == (5.0, 5000)
    assert np.array_equal(np.asarray(s.lower_bounds), [0.0, 0.0, 0.0, 0.01]) and np.array_equal(np.asarray(s.upper_bounds), [50.0, 50.0, 10.0, 0.01])
    assert np.array_equal(np.asarray(s.initial_step), [0.01] * 4) and s.dt is None and s.w is None and s.max_iters == 80


def test_build_pid_is_the_transfer_function(fb):
    p = (1.5, 2.5, 0.3, 0.04)
    A, B, Cm, D = fb.build_pid(p)
    for om in (0.1, 3.0, 200.0):
        s = 1j * om
        want = p[0] + p[1] / s + p[2] * s / (p[3] * s + 1)
        got = (Cm @ np.linalg.solve(s * np.eye(2) - A, B.astype(complex)) + D)[0, 0]
        assert abs(got - want) <= 1e-14 * abs(want)
        assert abs(proto.pid_response(np.array(p), np.array([om]))[0] - want) <= 1e-14 * abs(want)
    with pytest.raises(ValueError):
        fb.build_pid((1.0, 0.0, 0.0, 0.0))


# ---- 1. the prototype against the exact side ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", NX)
def test_prototype_agrees_with_the_exact_side(nx, capsys):
    n, m = 4, 3
    A, b, c, d = proto.plants(nx, n)
    P = proto.points(n, m)
    rep = lambda a: np.repeat(a, m, axis=0)
    Ab, bb, cb, db, Pb = rep(A), rep(b), rep(c), rep(d), P.reshape(-1, 4)
    for k in range(n * m):
        M = proto.closed_loop(Ab[k], bb[k], cb[k], db[k], Pb[k])[0]
        assert np.linalg.eigvals(M).real.max() < 0.0, (nx, k)
    pw = np.array([proto.freqresp(A[i], b[i], c[i], d[i], proto.W7) for i in range(n)])
    pe = np.array([proto.freqresp_exact(A[i], b[i], c[i], d[i], proto.W7) for i in range(n)])
    dfr = float((np.abs(pw - pe) / np.abs(pe)).max())
    got, cost, st = proto.metrics(Ab, bb, cb, db, Pb, proto.W7, 2.0, 1e-3)
    mapped, _, _ = proto.metrics(Ab, bb, cb, db, Pb, proto.W7, 2.0, 1e-3, side="map")
    want, _, ste = proto.metrics(Ab, bb, cb, db, Pb, proto.W7, 2.0, 1e-3, side="exact")
    dev, dmap = proto.rel_dev(got, want), proto.rel_dev(mapped, got)
    with capsys.disabled():
        print(f"\n[pid prototype vs exact] nx {nx:2d}, {n} x {m}: P(jw) {dfr:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in zip(("Ms", "ie", "ef", "iu", "up"), dev))
              + f"  (one-map form vs stage form {dmap.max():.1e})", end="")
    assert (st == 0).all() and (ste == 0).all()
    assert dfr <= 1e-12 and dev[0] <= 1e-12
    assert dev[1:].max() <= 1e-6, dev
    assert dmap.max() <= 1e-9
    assert np.allclose(cost, got.mean(axis=1), rtol=1e-15, atol=0.0)


def test_prototype_flags_the_failure_pairs():
    """1 / (s - 20) with p = (1, 0, 0, 0.01): the loop pole is +19, e^38 > 1e12 inside t_sim = 2; and d Dc = -1 exactly"""
    A = np.array([[[20.0]], [[-1.0]], [[-1.0]]]); b = np.ones((3, 1)); c = np.ones((3, 1)); d = np.array([0.0, 0.0, -0.5])
    P = np.array([[1.0, 0.0, 0.0, 0.01], [1.0, 1.0, 0.0, 0.01], [1.0, 0.0, 0.01, 0.01]])
    got, cost, st = proto.metrics(A, b, c, d, P, proto.W7, 2.0, 1e-3)
    assert st.tolist() == [proto.DIVERGED, 0, proto.SINGULAR]
    assert np.isinf(got[0, 1:]).all() and np.isfinite(got[0, 0]) and np.isinf(cost[0])
    assert np.isfinite(got[1]).all() and np.isfinite(cost[1])
    assert np.isnan(got[2]).all() and np.isinf(cost[2])


# ---- 2, 3. the reference's q2e loop on the oracle's Jacobian ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _q2e_plants(oracle):
    """A [28, 9, 9], b, c [28, 9], d [28]: trim and one-sided Jacobian of the oracle at the 28 nodes (as tests/test_reference_lqr_gains.py),
    the design model, te2te by scipy (reference_lqr.design), then the plant of c172x_design.jl:222-227"""
    tp = rf.design_trim_parameters_packed()
    env = oracle.default_env()
    ts0 = np.tile(np.array([0.1, 0.0, 0.75, 0.47, 0.014, -0.0015, 0.02])[:, None], (1, 28))
    assert oracle.lib.fo_set_kinematics(2) == 0
    try:
        r = oracle.trim(tp, ts0, env)
        assert r["ok"].all()

        def f_ode(X, U):
            m = X.shape[1]
            xd, y, st = oracle.f_ode(X, U, np.tile(r["ui"], m // 28), np.tile(r["s"], (1, m // 28)), env)
            assert (st == 0).all()
            return xd, y
        A, B, Cy = rl.linearize(f_ode, r["x"], r["u"])
    finally:
        oracle.lib.fo_set_kinematics(0)
    parts = []
    for k in range(28):
        Ap, Bp = rl.design_model(A[..., k], B[..., k], Cy[..., k])
        K_fbk, K_fwd, _ = rl.design("te2te", Ap, Bp)
        Ar, Br = rl._sub(Ap, Bp, rl.LON_RED, rl.U_LON)
        parts.append(proto.q2e_plant(Ar, Br, K_fbk, K_fwd, iq=rl.LON_RED.index("q"), i_ele=rl.U_LON.index("elevator_cmd")))
    out = tuple(np.array([p[j] for p in parts]) for j in range(4))
    for a in out:
        a.setflags(write=False)
    return out


def test_stored_q2e_gains_meet_the_references_thresholds(oracle, capsys):
    A, b, c, d = _q2e_plants(oracle)
    P = proto.q2e_stored()
    got, cost, st = proto.metrics(A, b, c, d, P, proto.Q2E_GRID, proto.Q2E_T_SIM, 1e-3, weights=proto.Q2E_WEIGHTS)
    lam = max(np.linalg.eigvals(proto.closed_loop(A[k], b[k], c[k], d[k], P[k])[0]).real.max() for k in range(28))
    with capsys.disabled():
        print(f"\n[q2e, stored gains, oracle Jacobian] worst over 28 nodes: Ms {got[:, 0].max():.4f}  ie {got[:, 1].max():.4f}  ef {got[:, 2].max():.4f}  "
              f"iu {got[:, 3].max():.4f}  up {got[:, 4].max():.3f}; cost {cost.min():.4f} .. {cost.max():.4f}; max Re lambda {lam:.1e}", end="")
    assert (st == 0).all()
    th = proto.Q2E_THRESHOLDS
    assert (got[:, 0] < th[0]).all() and (got[:, 1] < th[1]).all() and (got[:, 2] < th[2]).all()


def test_pattern_search_matches_the_references_optimum_at_node_13(fb, oracle, capsys):
    node, dt = 13, 2e-3
    A, b, c, d = (a[node:node + 1] for a in _q2e_plants(oracle))
    pw = proto.freqresp(A[0], b[0], c[0], d[0], proto.Q2E_GRID)
    calls = []

    def evaluate(pts):   # [1, m, 4] -> cost [1, m]
        m = pts.shape[1]
        rep = lambda a: np.repeat(a, m, axis=0)
        calls.append(m)
        return proto.metrics(rep(A), rep(b), rep(c), rep(d), pts[0], proto.Q2E_GRID, proto.Q2E_T_SIM, dt, weights=proto.Q2E_WEIGHTS,
                             side="map", Pw=rep(pw[None]))[1][None]
    x, f, evals, iters, done = fb.pidopt.pattern_search(evaluate, 1, proto.Q2E_DATA_0, proto.Q2E_LOWER, proto.Q2E_UPPER, 80)
    both = np.stack([x[0], proto.q2e_stored()[node], np.array(proto.Q2E_DATA_0)])
    rep3 = lambda a: np.repeat(a, 3, axis=0)
    met, cost, st = proto.metrics(rep3(A), rep3(b), rep3(c), rep3(d), both, proto.Q2E_GRID, proto.Q2E_T_SIM, dt, weights=proto.Q2E_WEIGHTS)
    with capsys.disabled():
        print(f"\n[q2e search, node {node}] {iters[0]} iterations, {evals[0]} evaluations: found {np.round(x[0], 4).tolist()} cost {cost[0]:.6f}; stored "
              f"{np.round(both[1], 4).tolist()} cost {cost[1]:.6f}; ratio {cost[0] / cost[1]:.5f}; data_0: Ms {met[2, 0]:.3f}", end="")
    assert (st == 0).all() and done[0] and iters[0] <= 80 and evals[0] == sum(calls)
    assert set(calls[1:]) == {12} and calls[0] == 1          # three free gains: 12 candidates per poll
    assert x[0, 3] == 0.01 and (x[0] >= proto.Q2E_LOWER).all() and (x[0] <= proto.Q2E_UPPER).all()
    assert abs(f[0] - cost[0]) <= 1e-9 * cost[0]             # (the search ran on the one-map form)
    assert cost[0] <= 1.01 * cost[1]
    assert fb.check_results(met[0], proto.Q2E_THRESHOLDS)
    assert met[2, 0] > 1.6 and not fb.check_results(met[2], proto.Q2E_THRESHOLDS)


# ---- 4. refusals that need no device -------------------------------------------------------------------------------------------------------------
class _World:
    n, nx, nu, ny = 3, 2, 1, 1
    u_labels, y_labels = ("u",), ("y",)
    _h = None


def test_host_refusals(fb):
    w = _World()
    ok = np.tile(np.array([1.0, 0.0, 0.0, 0.01]), (3, 2, 1))
    for bad, msg in ((np.ones((3, 2, 3)), "points must be"), (np.ones((2, 2, 4)), "points must be"), (np.ones((3, 65, 4)), "m = 65"),
                     (np.ones((3, 0, 4)), "m = 0")):
        with pytest.raises(ValueError, match=msg):
            fb.pid_metrics(w, bad)
    for tf in (0.0, -0.01, np.nan):
        p = ok.copy(); p[1, 1, 3] = tf
        with pytest.raises(ValueError, match="τ_f must be positive"):
            fb.pid_metrics(w, p)
    with pytest.raises(ValueError, match="input index 1"):
        fb.pid_metrics(w, ok, u=1)
    with pytest.raises(ValueError):
        fb.pid_metrics(w, ok, y="nope")
    S = fb.Settings
    for s, msg in ((S(w=np.array([1.0, 0.0])), "positive and finite"), (S(w=np.ones(1025)), "1 to 1024"), (S(w=np.ones((2, 2))), "1-D"),
                   (S(dt=0.0), "dt = 0"), (S(dt=1e-3, t_sim=1e-4), "at least dt"), (S(dt=1e-5, t_sim=10.0), "at most 200000")):
        with pytest.raises(ValueError, match=msg):
            fb.pid_metrics(w, ok, settings=s)
    for wt in (np.ones(4), [1, 1, 1, 1, -1], np.zeros(5), [1, 1, np.inf, 1, 1]):
        with pytest.raises(ValueError, match="weights"):
            fb.pid_metrics(w, ok, weights=wt)
    with pytest.raises(ValueError, match="frequency"):
        fb.freqresp(w, w=[])
    P = fb.PIDData
    with pytest.raises(ValueError, match="lower <= upper"):
        fb.optimize_pid(w, settings=S(lower_bounds=P(k_p=2.0, k_i=0, k_d=0, τ_f=0.01), upper_bounds=P(k_p=1.0, k_i=1, k_d=1, τ_f=0.01)))
    with pytest.raises(ValueError, match="τ_f"):
        fb.optimize_pid(w, settings=S(lower_bounds=P(k_p=0, k_i=0, k_d=0, τ_f=0.0), upper_bounds=P(k_p=1.0, k_i=1, k_d=1, τ_f=0.01)))
    with pytest.raises(ValueError, match="data_0"):
        fb.optimize_pid(w, data_0=np.ones((2, 4)))


def test_pattern_search_on_a_quadratic(fb):
    """four searches at once on |x - target|^2 inside the box: each ends at its own target (or at the bound nearest to it) to the step tolerance,
    a fixed dimension stays where it is, and an evaluation that returns +Inf never wins"""
    lo, hi = np.array([0.0, 0.0, 0.0, 0.01]), np.array([10.0, 50.0, 2.0, 0.01])
    target = np.array([[3.0, 20.0, 1.0, 0.01], [0.0, 50.0, 0.5, 0.01], [12.0, -5.0, 3.0, 0.01], [9.99, 0.01, 1.99, 0.01]])

    def evaluate(pts):
        c = (((pts - target[:, None, :]) / (hi - lo + 1.0)) ** 2).sum(axis=2)
        return np.where(pts[..., 0] > 9.995, np.inf, c)          # a forbidden strip
    x, f, evals, iters, done = fb.pidopt.pattern_search(evaluate, 4, (2.0, 15.0, 0.4, 0.01), lo, hi, 200)
    want = np.clip(target, lo, hi)
    want[2, 0] = 9.995
    assert done.all() and (iters < 200).all() and (evals == 1 + 12 * iters).all()
    assert (np.abs(x - want) <= 2e-4 * (hi - lo) + 1e-12).all(), x
    assert (x[:, 3] == 0.01).all() and np.isfinite(f).all()


def test_the_six_kernel_instances_are_in_the_library(fb, tmp_path_factory):
    """every instance the two entry points can launch is in the code object the host side was built with (a library whose host half knows
    a kernel its device half lacks aborts at the first launch), none uses scratch, and none is taken for a stepping instance"""
    from support import library_kernels
    kernels = library_kernels(tmp_path_factory)
    for P in (8, 16, 32):
        for name in (f"fbp::k_lss_freqresp<{P}>", f"fbp::k_pid_metrics<{P}>"):
            assert name in kernels, sorted(k for k in kernels if k.startswith("fbp::"))
            assert kernels[name]["scratch"] == 0 and kernels[name]["lds"] <= 160 * 1024 and "k_step_" not in name
        # the grid response works in fbq::Group's panels (csrc/lqr_kernels.hpp): per group of P lanes a P x (P + 1) panel and two side
        # panels of 8 x P / 2 doubles; 64 / P groups to a workgroup (the sampled twin keeps 5 P + 2 doubles: tests/test_dmargins_host.py)
        assert kernels[f"fbp::k_lss_freqresp<{P}>"]["lds"] == (P * (P + 1) + 2 * 8 * (P // 2)) * (64 // P) * 8
