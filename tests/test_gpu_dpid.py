"""fb_lss_dpid_metrics (flightbatch.dpid): optimize_PID's metrics under the sampled PID law for a batch of sampled models and PID candidates
on the device, and the pattern search on top of them, pinned by

  1. the exact side (a literal scalar transcription of the law, np.linalg.solve for P(z)) at every group edge, d = 0 and d > 0, tau_f = 0;
  2. bounded pairs: the clamp and halt counts as integers, the metrics, +-Inf bounds against no bounds, wave neighbours;
  3. position independence and reproducibility, bit for bit, and the handle left as it was;
  4. a diverging, a singular, a direct-feedthrough and a non-finite pair flagged in place among healthy ones;
  5. the device's other verbs: the loop closed on the host from build_dpid, stepped by timeresp.step and swept by dfreqresp;
  6. the refusals of the C ABI on a live device;
  7. the reference's stored q2e gains at the 28 design nodes under the law at 50 Hz, and optimize_dpid from them and from data_0.

The bound of 1, 2, 5 and 7 is the family's rule: the device differs from the numpy restatement of its algorithm (tests/dpid_prototype.py; held
to the exact side on the CPU by tests/test_dpid_host.py) in FMA contraction, summation order and <= 1-ulp division only, so its deviation
from the exact side may be ten times the prototype's over the same pairs, with the project's fp64 parity bound of 1e-11 as the floor. A
deviation is |got - exact| / |exact| per metric, the worst over the pairs. Ts = 0.02, t_sim = 2 (100 ticks), seven frequencies unless stated."""
import ctypes as C
import functools

import numpy as np
import pytest

import dpid_prototype as proto
import pid_prototype as pp
import reference_fixtures as rf
from support import pd

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-11, 10.0
NAMES = ("Ms", "ie", "ef", "iu", "up")
TS, T_SIM, N_TICKS = proto.TS, proto.T_SIM, int(round(proto.T_SIM / proto.TS))
IU, IY = 1, 2
pi32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
KEYS = ("metrics", "cost", "status", "counts")


def _world(fb, Phi, gam, c, d, seed=5, Ts=TS):
    """the plants as channel (IU, IY) of two-input, three-output sampled models whose other channels, and whose delta, x0, u0, y0, are random
    numbers (they play no part)"""
    n, nx = gam.shape
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, nx, 2)); B[:, :, IU] = gam
    Cm = rng.standard_normal((n, 3, nx)); Cm[:, IY, :] = c
    D = rng.standard_normal((n, 3, 2)); D[:, IY, IU] = d
    lss = fb.LinearizedSS(xdot0=rng.standard_normal((n, nx)), x0=rng.standard_normal((n, nx)), u0=rng.standard_normal((n, 2)),
                          y0=rng.standard_normal((n, 3)), A=Phi, B=B, C=Cm, D=D, x_labels=tuple(f"x{k}" for k in range(nx)),
                          u_labels=("other", "u"), y_labels=("y0", "y1", "y"))
    return fb.LinearWorld(lss, Ts=Ts)


def _run(fb, world, pts, bounds=None, weights=None, t_sim=T_SIM, w=None):
    return fb.dpid_metrics(world, pts, u=IU, y=IY, settings=fb.Settings(t_sim=t_sim), weights=weights, bounds=bounds, w=proto.W7() if w is None else w)


def _same(p, q, sel=slice(None)):
    return all(np.array_equal(getattr(p, k)[sel], getattr(q, k), equal_nan=True) for k in KEYS)


def _hold(tag, got, want, pro, capsys):
    """the rule of the module docstring per metric; prints the device's and the prototype's deviation"""
    dd, dp = proto.rel_dev(got, want), proto.rel_dev(pro, want)
    with capsys.disabled():
        print(f"\n[{tag}] " + "  ".join(f"{k} {a:.2e} ({b:.2e})" for k, a, b in zip(NAMES, dd, dp)), end="")
    for k, a, b in zip(NAMES, dd, dp):
        assert a <= max(MARGIN * b, FLOOR), (tag, k, a, b)


# ---- 1. the exact side at every group edge ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (3, 5), (9, 5), (130, 3)])
@pytest.mark.parametrize("nx", proto.NX_EDGES)
def test_metrics_against_the_exact_side(fb, nx, n, m, capsys):
    Phi, gam, c, d, P, pro, exact = proto.edge_reference(nx)
    weights = None if m == 1 else pp.Q2E_WEIGHTS
    w = _world(fb, Phi[:n], gam[:n], c[:n], d[:n])
    res = _run(fb, w, P[:n, :m], weights=weights)
    w.close()
    assert res.metrics.shape == (n, m, 5) and res.cost.shape == res.status.shape == (n, m) and res.counts.shape == (n, m, 2)
    assert (res.status == 0).all() and (res.counts == 0).all()
    assert n == 1 or ((d[:n] == 0).any() and (d[:n] > 0).any())
    _hold(f"fb_lss_dpid_metrics vs exact, nx {nx:2d}, {n} x {m}", res.metrics, exact[:n, :m], pro[:n, :m], capsys)
    wt = np.ones(5, dtype=np.longdouble) if weights is None else np.array(weights, dtype=np.longdouble)
    want = np.array((res.metrics.astype(np.longdouble) * wt).sum(axis=2) / wt.sum(), dtype=np.float64)
    assert (np.abs(res.cost - want) <= 1e-15 * want).all(), np.abs(res.cost / want - 1).max()


# ---- 2. bounded pairs ------------------------------------------------------------------------------------------------------------------------------
def test_bounded_pairs_counts_metrics_and_neighbours(fb, capsys):
    Phi, gam, c, d, P, lo, hi = proto.bounded_cases()
    pro, _, exact, counts, near = proto.bounded_reference()
    assert (near >= 1e-6).all()                                    # decided on the exact side (tests/test_dpid_host.py): the counts are integers to match
    w = _world(fb, Phi, gam, c, d)
    res = _run(fb, w, P, bounds=(lo, hi))
    assert (res.status == 0).all()
    assert np.array_equal(res.counts, counts), (res.counts - counts)
    _hold("fb_lss_dpid_metrics vs exact, bounded, nx 3", res.metrics, exact, pro, capsys)
    # bounds of +-Inf are no bounds, bit for bit
    none = _run(fb, w, P)
    inf = _run(fb, w, P, bounds=(-np.inf, np.inf))
    assert _same(none, inf) and (none.counts == 0).all() and (none.status == 0).all()
    # an unbounded pair keeps its bits whether or not its wave neighbours are bounded: every other candidate unbounded
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[:, 1::2], hi2[:, 1::2] = -np.inf, np.inf
    mixed = _run(fb, w, P, bounds=(lo2, hi2))
    w.close()
    for k in KEYS:
        assert np.array_equal(getattr(mixed, k)[:, 1::2], getattr(none, k)[:, 1::2]), k
        assert np.array_equal(getattr(mixed, k)[:, 0::2], getattr(res, k)[:, 0::2]), k
    assert (res.counts[:, 0::2, 0] >= 1).all()


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_independent_of_position_and_slot_and_repeatable(fb):
    n = 9
    Phi, gam, c, d, P, _, _ = proto.edge_reference(15)
    Phi, gam, c, P = Phi[:n], gam[:n], c[:n], P[:n]
    d = np.zeros(n)                                       # (so that half of the candidates can be bounded)
    lo, hi = np.full((n, 5), -np.inf), np.full((n, 5), np.inf)
    lo[:, 1], hi[:, 1], hi[:, 3] = -1.3, 1.3, 1.6
    run = lambda world, pts, b: _run(fb, world, pts, bounds=b, weights=pp.Q2E_WEIGHTS)
    w = _world(fb, Phi, gam, c, d)
    rng = np.random.default_rng(7)
    w.set_state(rng.standard_normal((15, n)))
    w.u = rng.standard_normal((2, n))
    w.step(7)
    w.sync()
    before = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model(), *w.model_cd(), w.Ts)
    first = run(w, P, (lo, hi))
    again = run(w, P, (lo, hi))
    after = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model(), *w.model_cd(), w.Ts)
    for p, q in zip(before, after):
        assert np.array_equal(p, q)
    assert before[2] == pytest.approx(7 * TS) and (first.status == 0).all() and first.counts[..., 0].max() >= 1
    assert _same(first, again)
    perm = np.array([3, 0, 4, 2, 1])
    assert _same(first, run(w, P[:, perm], (lo[:, perm], hi[:, perm])), (slice(None), perm))
    assert _same(first, run(w, P[:, 1:2], (lo[:, 1:2], hi[:, 1:2])), (slice(None), slice(1, 2)))
    assert _same(first, run(w, P[:, 2:3], (lo[:, 2:3], hi[:, 2:3])), (slice(None), slice(2, 3)))
    w.close()
    for pick in (np.arange(n)[::-1], np.array([8, 0, 5, 3])):
        ws = _world(fb, Phi[pick], gam[pick], c[pick], d[pick], seed=6)   # (other channels than the full batch's: they play no part)
        assert np.array_equal(ws.model()[0], before[4][pick])
        assert _same(first, run(ws, P[pick], (lo[pick], hi[pick])), pick)
        ws.close()


# ---- 4. failure pairs --------------------------------------------------------------------------------------------------------------------------------
def test_failure_pairs_are_flagged_in_place(fb):
    """Seven one-state plants, three candidates each (dpid_prototype.failure_pairs). System 2 has its pole at z = 1.5: with
    k_p = 0.1 in slot 1 the loop pole is 1.4 and 1.4^100 > 1e12 (its other candidates have k_p = 0.9: pole 0.6). System 5 has d = -0.5: with
    p = (2, 0, 0, tau_f) in slot 0, d Dc = -1 exactly. System 3 has d = 0.05 and a finite bound in slot 2. Then NaN in system 6's Phi. The
    inputs are fixed and nothing is retried: the overflow is arithmetic, by design of the input."""
    Phi, gam, c, d, P, lo, hi, expect = proto.failure_pairs()
    n, m = expect.shape
    pm, _, ps, _ = proto.metrics(*proto.pairs(Phi, gam, c, d, P), proto.W7(), TS, N_TICKS, lo.reshape(-1), hi.reshape(-1))
    assert np.array_equal(ps.reshape(n, m), expect)
    w = _world(fb, Phi, gam, c, d)
    res = _run(fb, w, P, bounds=(lo, hi))
    healthy, hlo, hhi = P.copy(), lo.copy(), hi.copy()
    healthy[2, 1] = P[2, 0]; healthy[5, 0] = P[5, 1]; hlo[3, 2], hhi[3, 2] = -np.inf, np.inf
    ref = _run(fb, w, healthy, bounds=(hlo, hhi))
    w.close()
    assert np.array_equal(res.status, expect), res.status
    assert (ref.status == 0).all() and np.isfinite(ref.metrics).all() and np.isfinite(ref.cost).all()
    dv = res.metrics[2, 1]
    assert np.isinf(dv[1:]).all() and (dv[1:] > 0).all() and np.isfinite(dv[0]) and res.cost[2, 1] == np.inf
    assert abs(dv[0] - pm.reshape(n, m, 5)[2, 1, 0]) <= 1e-12 * dv[0]          # Ms is still the grid's
    for i, j in ((5, 0), (3, 2)):
        assert np.isnan(res.metrics[i, j]).all() and res.cost[i, j] == np.inf and (res.counts[i, j] == 0).all()
    ok = expect == 0
    for k in KEYS:
        assert np.array_equal(getattr(res, k)[ok], getattr(ref, k)[ok]), k
    assert res.counts[4, 1, 0] >= 1
    # NaN in one Phi: that system's pairs are void (the grid response has no pivot), every other pair keeps its bits
    bad = Phi.copy(); bad[6, 0, 0] = np.nan
    wn = _world(fb, bad, gam, c, d)
    resn = _run(fb, wn, healthy, bounds=(hlo, hhi))
    wn.close()
    assert (resn.status[6] == proto.SINGULAR).all() and np.isnan(resn.metrics[6]).all() and np.isinf(resn.cost[6]).all() and (resn.counts[6] == 0).all()
    for k in KEYS:
        assert np.array_equal(getattr(resn, k)[:6], getattr(ref, k)[:6]), k


# ---- 5. against the device's other verbs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [7, 12])
def test_against_the_loop_closed_on_the_host_and_the_other_verbs(fb, nx, capsys):
    """unbounded pairs: the loop r -> (y, u, e) assembled on the host from build_dpid (dpid_prototype.closed_loop), one sampled model per pair,
    stepped by timeresp.step and swept by dfreqresp (|S| = 1 / |1 + P C| is the response r -> e); the metrics formed on the host"""
    n, m = 6, 2
    Phi, gam, c, d, P, pro, exact = proto.edge_reference(nx)
    w = _world(fb, Phi[:n], gam[:n], c[:n], d[:n])
    res = _run(fb, w, P[:n, :m])
    w.close()
    loops = [proto.closed_loop(Phi[i], gam[i], c[i], d[i], fb.build_dpid(P[i, j], TS)) for i in range(n) for j in range(m)]
    nz, z = nx + 2, np.zeros
    lss = fb.LinearizedSS(xdot0=z((n * m, nz)), x0=z((n * m, nz)), u0=z((n * m, 1)), y0=z((n * m, 3)), A=np.array([q[0] for q in loops]),
                          B=np.array([q[1] for q in loops]), C=np.array([q[2] for q in loops]), D=np.array([q[3] for q in loops]),
                          x_labels=tuple(f"z{k}" for k in range(nz)), u_labels=("r",), y_labels=("y", "u", "e"))
    wl = fb.LinearWorld(lss, Ts=TS)
    sr = fb.timeresp.step(wl, [("r", "y"), ("r", "u")], T_SIM)
    S = fb.dfreqresp(wl, "r", "e", proto.W7())                      # [nw, n m]
    wl.close()
    assert (sr.status == 0).all() and sr.y.shape == (n * m, 2, N_TICKS + 1)
    other = np.array([proto.host_metrics(sr.y[k, 0], sr.y[k, 1], S[:, k], N_TICKS) for k in range(n * m)]).reshape(n, m, 5)
    _hold(f"timeresp.step + dfreqresp of the closed loop vs exact, nx {nx}", other, exact[:n, :m], pro[:n, :m], capsys)
    _hold(f"fb_lss_dpid_metrics vs exact, nx {nx}", res.metrics, exact[:n, :m], pro[:n, :m], capsys)
    dev = proto.rel_dev(res.metrics, other)
    with capsys.disabled():
        print(f"\n[fb_lss_dpid_metrics vs the other verbs, nx {nx}] " + "  ".join(f"{k} {a:.2e}" for k, a in zip(NAMES, dev)), end="")


# ---- 6. refusals on a live device --------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_verb_and_the_cause_and_launch_nothing(fb):
    n, m, nw = 4, 2, 3
    grid = np.array([0.5, 1.0, 2.0])
    pts = np.tile(np.array([1.0, 0.5, 0.0, 0.02])[:, None, None], (1, m, n)).copy()        # [4 x m x N]
    bnd = np.stack([np.full((m, n), -2.0), np.full((m, n), 2.0)])                         # [2 x m x N]
    ones = np.ones(5)

    def call(h, iu=0, iy=0, w=grid, nw=nw, t_sim=1.0, weights=ones, pid=pts, bounds=None, m=m, metrics=True, cost=True, counts=True, status=True):
        mm = max(m, 1)
        met, co, cn, st = np.empty(5 * mm * n), np.empty(mm * n), np.empty(2 * mm * n, dtype=np.int32), np.empty(mm * n, dtype=np.int32)
        opt = lambda a: pd(a) if a is not None else None
        return fb.lib.fb_lss_dpid_metrics(h, iu, iy, opt(w), nw, t_sim, opt(weights), opt(pid), opt(bounds), m, pd(met) if metrics else None,
                                          pd(co) if cost else None, pi32(cn) if counts else None, pi32(st) if status else None)

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def refused(h, msg, **kw):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        rc = call(h, **kw)
        err = fb.lib.fb_last_error()
        assert rc != 0 and msg in err and b"fb_lss_dpid_metrics" in err, err
        assert launches(h) == 0

    Phi, gam, c, d = proto.dplants(3, n)
    w = proto.model(fb, Phi, gam, c, d)
    h = w._h
    neg_tau = pts.copy(); neg_tau[3, 1, 2] = -0.01
    nan_tau = pts.copy(); nan_tau[3, 0, 0] = np.nan
    inf_tau = pts.copy(); inf_tau[3, 0, 1] = np.inf
    eq_b = bnd.copy(); eq_b[1, 1, 3] = -2.0
    rev_b = bnd.copy(); rev_b[0, 0, 1] = 3.0
    nan_b = bnd.copy(); nan_b[1, 0, 2] = np.nan
    above = np.array([1.0, 2.0, 1.0001 * np.pi / TS])
    for kw, msg in ((dict(iu=1), b"iu = 1"), (dict(iu=-1), b"iu = -1"), (dict(iy=1), b"iy = 1"), (dict(w=None), b"grid w is required"),
                    (dict(nw=0), b"nw = 0"), (dict(w=np.ones(1025), nw=1025), b"nw = 1025"), (dict(w=np.array([1.0, 0.0, 2.0])), b"w[1]"),
                    (dict(w=np.array([1.0, 2.0, np.inf])), b"w[2]"), (dict(w=above), b"above the Nyquist frequency"),
                    (dict(m=0), b"m = 0"), (dict(m=65), b"m = 65"), (dict(t_sim=5e-3), b"1 <= N <= 200000"), (dict(t_sim=np.inf), b"t_sim = inf"),
                    (dict(t_sim=np.nan), b"t_sim = nan"), (dict(t_sim=4000.02), b"1 <= N <= 200000"), (dict(pid=neg_tau), b"tau_f = -0.01 at system 2, candidate 1"),
                    (dict(pid=nan_tau), b"tau_f = nan at system 0, candidate 0"), (dict(pid=inf_tau), b"tau_f = inf at system 1, candidate 0"),
                    (dict(bounds=eq_b), b"lo = -2, hi = -2 at system 3, candidate 1"), (dict(bounds=rev_b), b"lo = 3, hi = 2 at system 1, candidate 0"),
                    (dict(bounds=nan_b), b"hi = nan at system 2, candidate 0"),
                    (dict(weights=np.array([1.0, 1.0, -1.0, 1.0, 1.0])), b"weights[2]"), (dict(weights=np.zeros(5)), b"weights sum to zero"),
                    (dict(pid=None), b"are required"), (dict(cost=False), b"are required"), (dict(status=False), b"are required")):
        refused(h, msg, **kw)
    # and the handle still evaluates: two stamped launches (the grid response, then the metrics); null weights, metrics, counts and bounds
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert call(h, weights=None, metrics=False, counts=False) == 0, fb.lib.fb_last_error()
    assert launches(h) == 2
    assert call(h, bounds=bnd, t_sim=4000.0) == 0, fb.lib.fb_last_error()         # 200000 ticks, tau_f = 0.02, bounds
    # fb_pid_metrics keeps refusing the sampled handle, with the message it had
    met, co, st = np.empty(5 * m * n), np.empty(m * n), np.empty(m * n, dtype=np.int32)
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert fb.lib.fb_pid_metrics(h, 0, 0, pd(grid), nw, 1.0, 1e-2, pd(ones), pd(pts), m, pd(met), pd(co), pi32(st)) != 0
    assert b"fb_pid_metrics: a continuous-time verb on a sampled model" in fb.lib.fb_last_error()
    assert launches(h) == 0
    w.close()
    A, b, cc, dd = pp.plants(3, n)
    cont = fb.LinearWorld(pp.model(fb, A, b, cc, dd))
    refused(cont._h, b"a discrete-time verb on a continuous model")
    cont.close()
    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(ac._h, b"not a LinearizedSS handle")
    ac.close()
    hh = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 1, n, 0, C.byref(hh)) == 0
    refused(hh, b"no model yet")
    fb.lib.fb_destroy(hh)
    Phi, gam, c, d = proto.dplants(32, n)
    big = proto.model(fb, Phi, gam, c, d)
    refused(big._h, b"nx = 32")
    big.close()


# ---- 7. the reference's q2e loop under the law at 50 Hz, on the device from trim to metrics ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _q2e_sampled(fb):
    """Phi [28, 9, 9], gamma, c [28, 9], d [28] of the zero-order hold at Ts = 0.02 of P_q2e_opt (c172x_design.jl:222-227), and the continuous
    A, b: linearize at the 28 nodes, te2te by fb.lqr, K_fwd and the loop closed on the host (as tests/test_gpu_pid.py builds them), then c2d
    on the device"""
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
    parts = [pp.q2e_plant(Ar[k], Br[k], res.K[k], rl._k_fwd(Ar[k], Br[k], Cz, Dz, res.K[k]), iq=xl.index("q"), i_ele=ul.index("elevator_cmd"))
             for k in range(28)]
    A, b, c, d = (np.array([p[j] for p in parts]) for j in range(4))
    wc = fb.LinearWorld(pp.model(fb, A, b, c, d))
    sampled = fb.c2d(wc, TS)
    assert (sampled.status == 0).all()
    Phi, Gam = sampled.world.model()
    sampled.world.close()
    wc.close()
    out = (Phi, Gam[:, :, 0].copy(), c, d, A, b)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_q2e_table_under_the_flown_law(fb, capsys):
    Phi, gam, c, d, A, b = _q2e_sampled(fb)
    P = pp.q2e_stored()
    grid = fb.default_dgrid(TS)
    N = int(round(pp.Q2E_T_SIM / TS))
    w = proto.model(fb, Phi, gam, c, d)
    assert w.nx == 9 and w.Ts == TS
    res = fb.dpid_metrics(w, P[:, None, :], settings=fb.Settings(t_sim=pp.Q2E_T_SIM), weights=pp.Q2E_WEIGHTS)      # (the default grid)
    w.close()
    wc = fb.LinearWorld(pp.model(fb, A, b, c, d))
    cont = fb.pid_metrics(wc, P[:, None, :], settings=fb.Settings(t_sim=pp.Q2E_T_SIM, dt=1e-3, w=pp.Q2E_GRID), weights=pp.Q2E_WEIGHTS)
    wc.close()
    got, con = res.metrics[:, 0], cont.metrics[:, 0]
    th = pp.Q2E_THRESHOLDS
    with capsys.disabled():
        print("\n[q2e, stored gains, flown law at Ts = 0.02 | continuous] node | Ms | ie | ef | cost")
        for k in range(28):
            print(f"  {k:2d} | {got[k, 0]:.4f} {con[k, 0]:.4f} | {got[k, 1]:.4f} {con[k, 1]:.4f} | {got[k, 2]:.5f} {con[k, 2]:.5f} | {res.cost[k, 0]:.5f} {cont.cost[k, 0]:.5f}")
        print(f"  worst, flown law: Ms {got[:, 0].max():.4f}  ie {got[:, 1].max():.4f}  ef {got[:, 2].max():.5f}; continuous: Ms {con[:, 0].max():.4f}  "
              f"ie {con[:, 1].max():.4f}  ef {con[:, 2].max():.5f}; nodes inside Ms < {th[0]}, ie < {th[1]}, ef < {th[2]} under the flown law: "
              f"{int(fb.check_results(got, th).sum())} of 28", end="")
    assert (res.status == 0).all() and np.isfinite(res.metrics).all() and np.isfinite(res.cost).all() and (res.counts == 0).all()
    pro, _, st, _ = proto.metrics(Phi, gam, c, d, P, grid, TS, N, weights=pp.Q2E_WEIGHTS)
    exact, _, _ = proto.exact(Phi, gam, c, d, P, grid, TS, N)
    assert (st == 0).all()
    _hold("fb_lss_dpid_metrics vs exact, q2e, 28 nodes", got, exact, pro, capsys)


def test_optimize_dpid_on_the_28_q2e_plants(fb, capsys):
    Phi, gam, c, d, _, _ = _q2e_sampled(fb)
    stored = pp.q2e_stored()
    S, P = fb.Settings, fb.PIDData
    lower, upper = np.array(pp.Q2E_LOWER), np.array(pp.Q2E_UPPER)
    assert (stored >= lower).all() and (stored <= upper).all()          # (the search clips its start to the box: the stored gains lie inside)
    st = S(t_sim=pp.Q2E_T_SIM, lower_bounds=P(*lower), upper_bounds=P(*upper))
    wt = fb.Metrics(*pp.Q2E_WEIGHTS)
    w = proto.model(fb, Phi, gam, c, d)
    ref = fb.dpid_metrics(w, stored[:, None, :], settings=st, weights=wt)
    warm = fb.optimize_dpid(w, data_0=stored, settings=st, weights=wt)
    cold = fb.optimize_dpid(w, data_0=P(*pp.Q2E_DATA_0), settings=st, weights=wt)
    held = fb.optimize_dpid(w, data_0=stored, settings=st, weights=wt, bounds=(-1.0, 3.0))
    href = fb.dpid_metrics(w, stored[:, None, :], settings=st, weights=wt, bounds=(-1.0, 3.0))
    w.close()
    with capsys.disabled():
        print("\n[optimize_dpid, q2e, flown law] node | stored k_p k_i k_d | from stored: k_p k_i k_d, cost ratio, iterations | from data_0: cost ratio, iterations, evaluations")
        for k in range(28):
            print(f"  {k:2d} | {stored[k, 0]:7.4f} {stored[k, 1]:8.4f} {stored[k, 2]:7.4f} | {warm.data[k, 0]:7.4f} {warm.data[k, 1]:8.4f} {warm.data[k, 2]:7.4f} "
                  f"{warm.cost[k] / ref.cost[k, 0]:.5f} {warm.iters[k]:2d} | {cold.cost[k] / ref.cost[k, 0]:.5f} {cold.iters[k]:2d} {cold.evals[k]:4d}")
        print(f"  from stored: ratio {np.min(warm.cost / ref.cost[:, 0]):.5f} .. {np.max(warm.cost / ref.cost[:, 0]):.5f}, Ms <= {warm.metrics[:, 0].max():.4f}  "
              f"ie <= {warm.metrics[:, 1].max():.4f}  ef <= {warm.metrics[:, 2].max():.5f}; from data_0: ratio {np.min(cold.cost / ref.cost[:, 0]):.5f} .. "
              f"{np.max(cold.cost / ref.cost[:, 0]):.5f}, iterations {cold.iters.min()} - {cold.iters.max()}, evaluations {cold.evals.min()} - {cold.evals.max()}; "
              f"with the output held to [-1, 3]: ratio to the stored gains' bounded cost {np.min(held.cost / href.cost[:, 0]):.5f} .. {np.max(held.cost / href.cost[:, 0]):.5f}", end="")
    assert (ref.status == 0).all() and (warm.status == 0).all() and (href.status == 0).all() and (held.status == 0).all()
    assert (warm.cost <= ref.cost[:, 0]).all()          # the search never accepts a worse point
    assert (held.cost <= href.cost[:, 0]).all()
    assert (warm.iters <= 80).all() and (cold.iters <= 80).all() and (cold.status == 0).all()
    for r in (warm, cold, held):
        assert (r.data[:, 3] == 0.01).all() and (r.data >= lower).all() and (r.data <= upper).all()
