"""Margins on the device (fb_lss_margins; kernel: csrc/margins_kernels.hpp) against the exact side of tests/margins_prototype.py: LAPACK for
L, Brent's root finder inside the same grid brackets, closed forms where they exist.

The deviation rule is the family's (tests/test_gpu_connect.py): the device differs from the numpy restatement in FMA contraction, <= 1-ulp
division and its square root only, so it may deviate from the exact side ten times as far as the prototype does over the same systems, with
a floor of 1e-11. The scales: ω* relative, gm relative, pm in degrees divided by 180. tests/test_margins_host.py holds the prototype to the
exact side and checks that the cases are fair. Everything that says "the same" between two device runs is compared bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import margins_prototype as proto
from support import clock, gains_from_h5

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
pi = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
IU, IY = 1, 1


def _world(fb, systems):
    M = proto.lss_arrays(systems, iu=IU, iy=IY)
    nx = M["A"].shape[1]
    return fb.LinearWorld(fb.LinearizedSS(**M, x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=("u0", "u1"), y_labels=("y0", "y1")))


def _call(fb, world, w, gain=None, iu=IU, iy=IY, every=True):
    """the C call's own arrays: sel [10, N], counts [2, N], all [6, KMAX, N], status [N]"""
    n = world.n
    sel, counts, status = np.empty((10, n)), np.empty((2, n), dtype=np.int32), np.empty(n, dtype=np.int32)
    allv = np.empty((6, proto.KMAX, n)) if every else None
    g = None if gain is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64), (n,)))
    w = np.ascontiguousarray(w, dtype=np.float64)
    rc = fb.lib.fb_lss_margins(world._h, iu, iy, pd(w), w.size, pd(g), pd(sel), pi(counts), pd(allv), pi(status))
    assert rc == 0, fb.lib.fb_last_error()
    return sel, counts, allv, status


def _run(fb, systems, w, gain=None):
    world = _world(fb, systems)
    out = _call(fb, world, w, gain)
    world.close()
    return out


def _hold(label, out, refs, capsys):
    """out: the device's arrays; refs[i] = (prototype's deviation, exact result) of system i. The family's rule."""
    dev_d, dev_p = 0.0, 0.0
    for i, (dp, ex) in enumerate(refs):
        dev_d, dev_p = max(dev_d, proto.deviation(proto.from_device(*out, i), ex)), max(dev_p, dp)
    with capsys.disabled():
        print(f"\n[margins] {label}: device {dev_d:.2e}, prototype {dev_p:.2e}", end="")
    assert dev_d <= max(proto.FACTOR * dev_p, proto.FLOOR), (label, dev_d, dev_p)


def _ref(s, w, gain=1.0):
    ex = proto.exact(*s, w, gain)[0]
    return proto.deviation(proto.margins(*s, w, gain), ex), ex


# ---- 1. closed forms at every group size ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closed_refs(nx):
    return [_ref(s, proto.W_CLOSED) for s, _ in proto.closed_systems(nx)]


def _form(sel, K):
    """the worst deviation of gm, wpc, pm, wgc from the closed forms of K / (s + 1)³"""
    gm, wpc, pm, wgc = proto.cube_closed_form(K)
    return max(abs(sel[0] / gm - 1.0), abs(sel[1] / wpc - 1.0), abs(sel[2] - pm) / 180.0, abs(sel[3] / wgc - 1.0))


@functools.lru_cache(maxsize=None)
def _closed_form_proto(nx):
    return max(_form(proto.margins(*s, proto.W_CLOSED)[0], K) for s, K in proto.closed_systems(nx))


@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("nx", proto.NX_CLOSED)
def test_closed_forms(fb, nx, n, capsys):
    distinct, refs = proto.closed_systems(nx), _closed_refs(nx)
    pick = [i % len(distinct) for i in range(n)]
    out = _run(fb, [distinct[k][0] for k in pick], proto.W_CLOSED)
    assert (out[3] == 0).all() and (out[1] == 1).all()
    _hold(f"K / (s + 1)³ in nx = {nx:2d}, {n:3d} systems", out, [refs[k] for k in pick], capsys)
    dev_d = max(_form(out[0][:, i], distinct[k][1]) for i, k in enumerate(pick))
    dev_p = _closed_form_proto(nx)
    with capsys.disabled():
        print(f"; closed forms: device {dev_d:.2e}, prototype {dev_p:.2e}", end="")
    assert dev_d <= max(proto.FACTOR * dev_p, proto.FLOOR)


# ---- 2. small and degenerate plants --------------------------------------------------------------------------------------------------------------
def test_small_and_degenerate_plants(fb, capsys):
    w = np.logspace(-2.0, 2.0, 65)
    for label, kinds in (("nx = 1", [proto.tf([3.0], [1.0, 1.0]), proto.tf([0.5], [1.0, 1.0])]),
                         ("nx = 2", [proto.tf([3.0], [1.0, 1.0, 0.0]), proto.tf([0.4], [1.0, 1.0, 0.0])])):
        systems = [kinds[i % 2] for i in range(9)]
        out = _run(fb, systems, w)
        _hold(label, out, [_ref(s, w) for s in systems], capsys)
        sel, counts, allv, status = out
        assert (status == 0).all() and (counts[0] == 0).all() and (sel[0] == np.inf).all() and np.isnan(sel[[1, 4, 5]]).all()
        if label == "nx = 1":      # K / (s + 1): a gain crossing only when K > 1; 0.5 / (s + 1) has no crossing of either kind
            assert counts[1].tolist() == [1, 0] * 4 + [1]
            assert (sel[2, 1::2] == np.inf).all() and np.isnan(sel[3, 1::2]).all() and np.isnan(allv[:, :, 1::2]).all()
            assert (sel[9, 1::2] == w[-1]).all()
        else:                      # K / (s (s + 1)): A is singular, one gain crossing, no phase crossing
            assert (counts[1] == 1).all()


# ---- 3. unequal work inside one wave -------------------------------------------------------------------------------------------------------------
def test_unequal_work_inside_one_wave(fb, capsys):
    named = proto.work_systems()
    systems, w = [s for _, s in named], proto.W_WORK
    big = _run(fb, systems, w)
    want = {"none": (0, 0), "one": (0, 1), "two": (1, 1), "three": (2, 1), "first-order": (0, 1)}
    assert (big[3] == 0).all() and [tuple(big[1][:, i]) for i in range(len(named))] == [want[k] for k, _ in named]
    assert (big[0][0, [i for i, (k, _) in enumerate(named) if k == "three"]] < 1.0).all()      # conditionally stable: a gain reduction margin
    _hold(f"0 to 3 crossings in nx = {proto.NX_WORK}", tuple(a[..., :10] for a in big), [_ref(s, w) for s in systems[:10]], capsys)
    take = lambda out, idx: tuple(a[..., idx] for a in out)
    for i in list(range(12)) + [63, 64, 129]:          # each system alone
        assert same(_run(fb, [systems[i]], w), take(big, [i])), i
    assert same(take(_run(fb, systems[::-1], w), np.arange(len(systems))[::-1]), big)
    world = _world(fb, systems)
    first, second = _call(fb, world, w), _call(fb, world, w)
    world.close()
    assert same(first, big) and same(second, big)
    for n in (1, 3, 9, 63):
        assert same(_run(fb, systems[:n], w), take(big, np.arange(n))), n


# ---- 4. grid edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [65, 70, 130])
def test_crossings_in_the_first_and_the_last_interval(fb, nw, capsys):
    for K in proto.K_CLOSED:
        s, w = proto.cube(K), proto.edge_grid(K, nw)
        out = _run(fb, [s] * 3, w)
        assert (out[3] == 0).all() and (out[1] == 1).all()
        assert (out[2][0, 0] > w[-2]).all() and (out[2][3, 0] < w[1]).all()
        _hold(f"{nw} frequencies, K = {K:g}", out, [_ref(s, w)] * 3, capsys)


def test_a_grid_response_that_takes_two_launches(fb):
    """2^16 + 1 systems of 17 states (two to a workgroup) on 1024 frequencies pass the 2^25 workgroups one launch of stage 1 holds: the grid
    response runs as 1023 frequencies and then one, and every row is what it is in a small batch (the crossings lie in the second half
    of the grid, the last frequency is its own slice)"""
    n, w = (1 << 16) + 1, np.logspace(-2.0, 2.0, 1024)
    distinct = [s for s, _ in proto.closed_systems(17)]
    M = proto.lss_arrays(distinct, iu=IU, iy=IY)
    idx = np.arange(n) % len(distinct)
    world = fb.LinearWorld(fb.LinearizedSS(**{k: v[idx] for k, v in M.items()}, x_labels=tuple(f"x{k}" for k in range(17)), u_labels=("u0", "u1"),
                                           y_labels=("y0", "y1")))
    assert fb.lib.fb_timing_begin_per_launch(world._h, 8) == 0
    big = _call(fb, world, w)
    ms, nl = C.c_float(), C.c_int64(-1)
    assert fb.lib.fb_timing_end(world._h, C.byref(ms), C.byref(nl)) == 0 and fb.lib.fb_timing_launches(world._h, None, 0, C.byref(nl)) == 0
    world.close()
    assert nl.value == 3
    small = _run(fb, distinct, w)
    assert (small[3] == 0).all() and (small[1] == 1).all()
    for lo in (0, 12 * 2730, n - 1 - (n - 1) % 12 - 12):          # the first, a middle and the last full cycle of the 12 distinct systems
        assert lo % 12 == 0 and same(tuple(a[..., lo:lo + 12] for a in big), small), lo
    assert (big[3] == 0).all() and (big[1] == 1).all()


# ---- 5. more crossings than are kept ---------------------------------------------------------------------------------------------------------------
def test_more_than_kmax_crossings(fb, capsys):
    rng = np.random.default_rng(3)
    s, other = proto.modes(), proto.embed(proto.cube(4.0), 12, rng)
    systems, w = [s, other, s], proto.W_MODES
    sel, counts, allv, status = out = _run(fb, systems, w)
    assert status.tolist() == [proto.TRUNCATED, 0, proto.TRUNCATED] and counts[:, 0].tolist() == [0, proto.KMAX] and counts[:, 1].tolist() == [1, 1]
    assert (np.diff(allv[3, :, 0]) > 0.0).all() and np.isfinite(allv[3:, :, 0]).all() and np.isnan(allv[:3, :, 0]).all()
    _hold("six lightly damped modes", out, [_ref(x, w) for x in systems], capsys)


# ---- 6. the gain -----------------------------------------------------------------------------------------------------------------------------------
def test_gain(fb, capsys):
    s, w = proto.closed_systems(9)[1][0], proto.W_CLOSED
    one, k = _run(fb, [s], w), _run(fb, [s], w, 0.6)
    _hold("gain 0.6", k, [_ref(s, w, 0.6)], capsys)
    dp = proto.deviation(proto.margins(*s, w, 0.6), proto.exact(*s, w, 0.6)[0]) + proto.deviation(proto.margins(*s, w), proto.exact(*s, w)[0])
    bound = max(proto.FACTOR * dp, proto.FLOOR)
    assert abs(k[0][0, 0] / (one[0][0, 0] / 0.6) - 1.0) <= bound and abs(k[0][1, 0] / one[0][1, 0] - 1.0) <= bound
    gains = np.array([1.0, 0.6, 2.0, 0.3, 1.5])
    batch = _run(fb, [s] * 5, w, gains)
    for i, g in enumerate(gains):
        assert same(_run(fb, [s], w, g), tuple(a[..., [i]] for a in batch)), g
    assert same(tuple(a[..., [0]] for a in batch), one)          # a NULL gain is ones


# ---- 7. bad inputs among healthy neighbours ---------------------------------------------------------------------------------------------------------
def test_bad_inputs_among_healthy_neighbours(fb):
    w = np.array([0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0])
    healthy = [proto.tf([1.0 + 0.5 * i], [1.0, 1.0 + 0.1 * i, 0.0]) for i in range(9)]
    clean = _run(fb, healthy, w)
    assert (clean[3] == 0).all() and (clean[1][1] == 1).all()
    bad = list(healthy)
    A = healthy[2][0].copy(); A[1, 0] = np.nan
    bad[2] = (A,) + healthy[2][1:]
    bad[6] = (np.array([[0.0, 1.0], [-1.0, 0.0]]),) + healthy[6][1:]          # jωI - A is singular at ω = 1, which the grid holds
    gains = np.ones(9); gains[4] = np.nan
    world = _world(fb, bad)
    world.step(7, dt=1e-3)
    world.sync()
    snap = lambda: (world.x, world.u, *clock(fb, world), world.status, *world.model(), *world.model_cd(), world.params.dt)
    before = snap()
    sel, counts, allv, status = _call(fb, world, w, gains)
    after = snap()
    world.close()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    assert status.tolist() == [0, 0, proto.NOT_FINITE, 0, proto.NOT_FINITE, 0, proto.SINGULAR, 0, 0]
    for i in (2, 4, 6):
        assert np.isnan(sel[:, i]).all() and np.isnan(allv[:, :, i]).all() and (counts[:, i] == 0).all()
    ok = [0, 1, 3, 5, 7, 8]
    assert same(tuple(a[..., ok] for a in (sel, counts, allv, status)), tuple(a[..., ok] for a in clean))


# ---- 8. the notebook's position loop ------------------------------------------------------------------------------------------------------------------
def _velocity_loop(fb, n=3):
    w = fb.Robot2DWorld(n)
    fb.linearize(w, None, scheme="forward")
    plant = fb.linear_world(w)
    w.close()
    g = gains_from_h5()
    K_x, K_fwd, K_int = g[0:3], g[3], g[4]
    integ = fb.integrator_world(n)
    F = np.array([[-K_x[0], -K_x[1], -K_x[2], -1.0], [0.0, K_int, 0.0, 0.0]])
    vel = fb.connect(plant, integ, feedback=F, inputs=np.array([[K_fwd], [-K_int]]), reads=["ω", "v", "θ", "ξ"], input_labels=("v_ref",))
    plant.close(); integ.close()
    assert vel.ok.all()
    return vel.world


def test_the_notebooks_position_loop(fb, capsys):
    vel = _velocity_loop(fb)
    A, B = vel.model()
    Cm, D = vel.model_cd()
    iu, iy = vel.u_labels.index("v_ref"), vel.y_labels.index("η")
    s = (A[0], B[0][:, iu], Cm[0][iy], D[0][iy, iu])
    w = fb.pidopt.default_grid()
    for gain in (1.0, 0.6):
        res = fb.margins(vel, u="v_ref", y="η", gain=None if gain == 1.0 else gain, all=True)
        out = _call(fb, vel, w, None if gain == 1.0 else gain, iu=iu, iy=iy)
        assert np.array_equal(res.gm, out[0][0]) and np.array_equal(res.pm, out[0][2]) and np.array_equal(res.wgc_all, out[2][3].T, equal_nan=True)
        assert res.ok.all() and (res.npc >= 1).all() and (res.ngc >= 1).all()
        _hold(f"the position loop, k_p = {gain:g}", out, [_ref(s, w, gain)] * vel.n, capsys)
        with capsys.disabled():
            print("\n    " + res.show(0), end="")
        assert np.allclose(res.ms, 1.0 / out[0][8]) and np.array_equal(res.gm_db, 20.0 * np.log10(res.gm))
    vel.close()


# ---- 9. the q2e loop at three of the 28 design nodes --------------------------------------------------------------------------------------------------
def test_the_q2e_loop_at_design_nodes(fb, capsys):
    import pid_prototype
    import reference_fixtures as rf
    import reference_lqr as rl
    EAS, h, flaps = rf.design_nodes()
    cw = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(cw, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme="onesided2")
    cw.close()
    assert lss.success.all() and (lss.status == 0).all()
    rows = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    xl, ul, zl, qx, _, r, _ = rl.DESIGNS["te2te"]
    red = [rl._sub(*rl.design_model(lss.A[k], lss.B[k], lss.C[k][rows]), xl, ul) for k in range(28)]
    Ar, Br = np.array([p[0] for p in red]), np.array([p[1] for p in red])
    lw = fb.LinearWorld(fb.design_model(Ar, Br, x_labels=xl, u_labels=ul))
    res = fb.lqr(lw, [float(qx.get(k, 0.0)) for k in xl], np.array(r, dtype=np.float64))
    assert (res.status == 0).all()
    Cz, Dz = rl._z_rows(xl, ul, zl)
    Kf = np.array([rl._k_fwd(Ar[k], Br[k], Cz, Dz, res.K[k]) for k in range(28)])
    nx, nu = len(xl), len(ul)
    F = np.zeros((28, nu + 1, nx + 1))
    F[:, :nu, :nx] = -res.K
    F[:, :nu, nx] = Kf[:, :, ul.index("elevator_cmd")]
    G = np.zeros((nu + 1, 1)); G[nu, 0] = 1.0
    integ = fb.integrator_world(28)
    q2e = fb.connect(lw, integ, feedback=F, inputs=G, outputs=["q"], input_labels=("q_err",))
    assert q2e.ok.all()
    P = pid_prototype.q2e_stored()
    pid = fb.pid_world(np.asarray(P, dtype=np.float64))
    # the open loop L = P_q2e C_q2e: the PID in series with the plant
    series = fb.connect(q2e.world, pid, feedback=np.array([[0.0, 1.0], [0.0, 0.0]]), inputs=np.array([[0.0], [1.0]]), input_labels=("e",))
    assert series.ok.all()
    sw = series.world
    iy = sw.y_labels.index("q")
    w = fb.pidopt.default_grid()
    out = _call(fb, sw, w, iu=0, iy=iy)
    A, B = sw.model()
    Cm, D = sw.model_cd()
    nodes = [0, 14, 27]
    assert (out[3][nodes] == 0).all()
    _hold("q2e loop at design nodes 0, 14, 27", tuple(a[..., nodes] for a in out), [_ref((A[k], B[k][:, 0], Cm[k][iy], D[k][iy, 0]), w) for k in nodes], capsys)
    with capsys.disabled():
        for k in nodes:
            print(f"\n    node {k:2d}: GM {out[0][0, k]:.3f} at {out[0][1, k]:.3f} rad/s, PM {out[0][2, k]:.2f}° at {out[0][3, k]:.3f} rad/s, "
                  f"Ms {1.0 / out[0][8, k]:.3f}", end="")
    for x in (lw, integ, q2e.world, pid, sw):
        x.close()


# ---- 10. refusals and the example -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n, grid = 5, np.logspace(-1.0, 1.0, 17)
    world = _world(fb, [proto.cube(4.0)] * n)
    sel, counts, status, allv = np.empty((10, n)), np.empty((2, n), dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((6, proto.KMAX, n))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64(-1)
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def call(h, iu=IU, iy=IY, w=grid, nw=None, sel=sel, counts=counts, status=status):
        return fb.lib.fb_lss_margins(h, iu, iy, pd(w), (0 if w is None else w.size) if nw is None else nw, None, pd(sel), pi(counts), pd(allv), pi(status))

    def refused(h, cause, timed=True, **kw):
        if timed:
            assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        rc = call(h, **kw)
        err = fb.lib.fb_last_error()
        assert rc != 0 and cause in err, (cause, err)
        assert not timed or (b"fb_lss_margins" in err and launches(h) == 0), err

    refused(None, b"null handle", timed=False)
    r = fb.Robot2DWorld(n)
    refused(r._h, b"not a LinearizedSS handle", timed=False)          # (a Robot2D handle keeps no per-launch stamps)
    r.close()
    hh = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 2, 2, n, 0, C.byref(hh)) == 0
    refused(hh, b"no model yet")
    fb.lib.fb_destroy(hh)
    sampled = fb.c2d(world, 0.01).world
    refused(sampled._h, b"a continuous-time verb on a sampled model")
    sampled.close()
    h = world._h
    refused(h, b"iu = 2 is outside", iu=2)
    refused(h, b"iu = -1 is outside", iu=-1)
    refused(h, b"iy = 2 is outside", iy=2)
    refused(h, b"the frequency grid w is required", w=None, nw=17)
    refused(h, b"sel, counts and status are required", sel=None)
    refused(h, b"sel, counts and status are required", counts=None)
    refused(h, b"sel, counts and status are required", status=None)
    refused(h, b"nw = 1,", nw=1)
    refused(h, b"nw = 1025,", w=np.logspace(-1, 1, 1025))
    for k, v in ((3, 0.0), (3, -1.0), (3, np.inf), (3, np.nan)):
        g = grid.copy(); g[k] = v
        refused(h, b"must be positive and finite", w=g)
    g = grid.copy(); g[5] = g[4]
    refused(h, b"the grid must strictly increase", w=g)
    refused(h, b"the grid must strictly increase", w=grid[::-1].copy())
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert call(h) == 0 and launches(h) == 2          # the grid response, then the margins
    with pytest.raises(ValueError, match="strictly increasing"):
        fb.margins(world, w=grid[::-1])
    with pytest.raises(ValueError, match="2 to 1024"):
        fb.margins(world, w=grid[:1])
    world.close()
    # N nw above 2^31 - 1: 2^21 systems of one state on 1024 frequencies
    big_n = 1 << 21
    z, o = np.zeros((big_n, 1)), np.ones((big_n, 1, 1))
    big = fb.LinearWorld(fb.LinearizedSS(xdot0=z, x0=z, u0=z, y0=z, A=-o, B=o, C=o, D=0.0 * o, x_labels=("x",), u_labels=("u",), y_labels=("y",)))
    assert fb.lib.fb_timing_begin_per_launch(big._h, 8) == 0
    rc = fb.lib.fb_lss_margins(big._h, 0, 0, pd(np.logspace(-1, 1, 1024)), 1024, None, pd(sel), pi(counts), None, pi(status))
    err = fb.lib.fb_last_error()
    assert rc != 0 and b"exceed the 2^31 - 1 pairs" in err and launches(big._h) == 0, err
    big.close()


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "loop_margins.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GM" in r.stdout and "PM" in r.stdout and "stable" in r.stdout
