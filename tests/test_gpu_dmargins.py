"""Sampled loops on the device (fb_lss_set_sampled, fb_lss_dfreqresp, fb_lss_dmargins, fb_lss_dpoles; kernels: csrc/dfreq_kernels.hpp and
fbe::k_poles) against the exact side of tests/dmargins_prototype.py: LAPACK for L, Brent's root finder on θ inside the same grid brackets,
closed forms where they exist.

The deviation rule is the family's (tests/test_gpu_margins.py): the device differs from the numpy restatement in FMA contraction, <= 1-ulp
division and its square root only, so it may deviate from the exact side ten times as far as the prototype does over the same systems, with
a floor of 1e-11. The scales: ω* relative, gm relative, pm in degrees divided by 180. tests/test_dmargins_host.py holds the prototype to the
exact side and checks that the cases are fair. Where a world comes from fb_lss_c2d the exact side is computed from the device's own Φ, Γ,
read back: c2d's error is not this file's. Everything that says "the same" between two device runs is compared bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import dmargins_prototype as proto
import margins_prototype as mp
import poles_prototype as pp
from support import clock

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
pi = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
bits = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
take = lambda out, idx: tuple(a[..., idx] for a in out)
IU, IY = 1, 1
TS = proto.TS_CLOSED


def _lss(fb, systems, **kw):
    M = proto.lss_arrays(systems, iu=IU, iy=IY, **kw)
    nx = M["A"].shape[1]
    return fb.LinearizedSS(**M, x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=("u0", "u1"), y_labels=("y0", "y1"))


def _given(fb, systems, Ts):
    """a sampled world of systems given as (Φ, γ, c, d): LinearWorld(lss, Ts=...)"""
    return fb.LinearWorld(_lss(fb, systems), Ts=Ts)


def _held(fb, systems, Ts):
    """the zero-order hold of continuous systems, made on the device"""
    src = fb.LinearWorld(_lss(fb, systems))
    res = fb.c2d(src, Ts)
    src.close()
    assert (res.status == 0).all()
    return res.world


def _systems(world):
    """the channel's (Φ, γ, c, d) of every system as the device holds them"""
    Phi, Gam = world.model()
    Cm, D = world.model_cd()
    return [(Phi[i], Gam[i][:, IU].copy(), Cm[i][IY].copy(), float(D[i][IY, IU])) for i in range(world.n)]


def _call(fb, world, w, gain=None, iu=IU, iy=IY, every=True):
    """the C call's own arrays: sel [10, N], counts [2, N], all [6, KMAX, N], status [N]"""
    n = world.n
    sel, counts, status = np.empty((10, n)), np.empty((2, n), dtype=np.int32), np.empty(n, dtype=np.int32)
    allv = np.empty((6, proto.KMAX, n)) if every else None
    g = None if gain is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64), (n,)))
    w = np.ascontiguousarray(w, dtype=np.float64)
    rc = fb.lib.fb_lss_dmargins(world._h, iu, iy, pd(w), w.size, pd(g), pd(sel), pi(counts), pd(allv), pi(status))
    assert rc == 0, fb.lib.fb_last_error()
    return sel, counts, allv, status


def _run(fb, systems, w, Ts=TS, gain=None):
    world = _given(fb, systems, Ts)
    out = _call(fb, world, w, gain)
    world.close()
    return out


def _run_held(fb, systems, w, Ts, gain=None):
    world = _held(fb, systems, Ts)
    out = _call(fb, world, w, gain)
    world.close()
    return out


def _hold(label, out, refs, capsys):
    """out: the device's arrays; refs[i] = (prototype's deviation, exact result, prototype's result) of system i. The family's rule."""
    dev_d, dev_p, dev_dp = 0.0, 0.0, 0.0
    for i, (dp, ex, pr) in enumerate(refs):
        got = proto.from_device(*out, i)
        dev_d, dev_p, dev_dp = max(dev_d, proto.deviation(got, ex)), max(dev_p, dp), max(dev_dp, proto.deviation(got, pr))
    with capsys.disabled():
        print(f"\n[dmargins] {label}: device vs exact {dev_d:.2e}, prototype vs exact {dev_p:.2e}, device vs prototype {dev_dp:.2e}", end="")
    assert dev_d <= max(proto.FACTOR * dev_p, proto.FLOOR), (label, dev_d, dev_p)


def _ref(s, w, Ts=TS, gain=1.0):
    ex, pr = proto.exact(*s, w, Ts, gain)[0], proto.margins(*s, w, Ts, gain)
    return proto.deviation(pr, ex), ex, pr


def _launches(fb, h):
    ms, nl = C.c_float(), C.c_int64(-1)
    assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
    assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
    return nl.value


# ---- 1. closed forms at every group edge ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closed_refs(nx):
    return [_ref(s, proto.W_CLOSED) for s, _ in proto.closed_systems(nx)]


def _form(sel, K):
    """the worst deviation of gm, wpc, pm, wgc from the closed forms of K / (z (z - 1))"""
    gm, wpc, pm, wgc = proto.delay_closed_form(K, TS)
    return max(abs(sel[0] / gm - 1.0), abs(sel[1] / wpc - 1.0), abs(sel[2] - pm) / 180.0, abs(sel[3] / wgc - 1.0))


@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("nx", proto.NX_CLOSED)
def test_closed_forms(fb, nx, n, capsys):
    distinct, refs = proto.closed_systems(nx), _closed_refs(nx)
    pick = [i % len(distinct) for i in range(n)]
    world = _given(fb, [distinct[k][0] for k in pick], TS)          # Φ has an eigenvalue at 0: no c2d makes this world
    assert world.Ts == TS
    out = _call(fb, world, proto.W_CLOSED)
    world.close()
    assert (out[3] == 0).all() and (out[1] == 1).all()
    _hold(f"K / (z (z - 1)) in nx = {nx:2d}, {n:3d} systems", out, [refs[k] for k in pick], capsys)
    dev_d = max(_form(out[0][:, i], distinct[k][1]) for i, k in enumerate(pick))
    dev_p = max(_form(refs[k][2][0], distinct[k][1]) for k in range(len(distinct)))
    with capsys.disabled():
        print(f"; closed forms: device {dev_d:.2e}, prototype {dev_p:.2e}", end="")
    assert dev_d <= max(proto.FACTOR * dev_p, proto.FLOOR)


# ---- 2. the c2d chain ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ts", [0.05, 0.5])
def test_the_c2d_chain(fb, Ts, capsys):
    rng = np.random.default_rng(9)
    cont = [mp.embed(proto.cube(K), 9, rng) for K in mp.K_CLOSED for _ in range(3)]
    world = _held(fb, cont, Ts)
    w = proto.w_zoh(Ts)
    out = _call(fb, world, w)
    sampled = _systems(world)
    res = fb.dmargins(world, u=IU, y=IY, w=w, all=True)
    world.close()
    assert (out[3] == 0).all() and (out[1] == 1).all()
    assert np.array_equal(res.gm, out[0][0]) and np.array_equal(res.pm, out[0][2]) and np.array_equal(res.wpc_all, out[2][0].T, equal_nan=True)
    _hold(f"c2d of K / (s + 1)³ in nx = 9 at Ts = {Ts:g}", out, [_ref(s, w, Ts) for s in sampled], capsys)
    for i, s in enumerate(cont):          # against the continuous loop: the hold costs about ω_gc Ts / 2 of phase margin and some gain margin
        gm, wpc, pm, wgc = mp.cube_closed_form(mp.K_CLOSED[i // 3])
        assert out[0][0, i] < gm and 0.0 < pm - out[0][2, i] < 2.0 * np.degrees(wgc * Ts / 2.0) + 1.0


# ---- 3. fb_lss_dfreqresp ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _freq_refs(nx):
    """(exact, prototype) [12, 33] of the distinct closed-form systems on W_CLOSED"""
    distinct = [s for s, _ in proto.closed_systems(nx)]
    ex = np.array([[proto.exact_response(*s, complex(np.cos(t), np.sin(t))) for t in proto.W_CLOSED * TS] for s in distinct])
    return ex, np.array([proto.dfreqresp(*s, proto.W_CLOSED, TS) for s in distinct])


def _fma_sq(a, b):
    """fma(a, a, b * b), exactly rounded"""
    return float(Fraction(a) * Fraction(a) + Fraction(b * b))


@pytest.mark.parametrize("nx", proto.NX_CLOSED)
def test_dfreqresp_against_lapack(fb, nx, capsys):
    n = 130
    distinct = [s for s, _ in proto.closed_systems(nx)]
    pick = np.arange(n) % len(distinct)
    world = _given(fb, [distinct[k] for k in pick], TS)
    ex, pr = _freq_refs(nx)
    full = fb.dfreqresp(world, IU, IY, proto.W_CLOSED)
    one = fb.dfreqresp(world, IU, IY, proto.W_CLOSED[16:17])
    wide = fb.dfreqresp(world, IU, IY, np.repeat(proto.W_CLOSED, 2)[:65])          # 65 frequencies (the response takes a grid that repeats)
    assert full.shape == (33, n) and one.shape == (1, n) and wide.shape == (65, n)
    assert np.array_equal(one[0], full[16]) and np.array_equal(wide[0::2], full) and np.array_equal(wide[1::2], full[:32])
    dev_d, dev_p = np.abs(full / ex[pick].T - 1.0).max(), np.abs(pr / ex - 1.0).max()
    with capsys.disabled():
        print(f"\n[dfreqresp] nx = {nx:2d}, {n} systems x 33: device vs LAPACK {dev_d:.2e}, prototype {dev_p:.2e}, device vs prototype "
              f"{np.abs(full / pr[pick].T - 1.0).max():.2e}", end="")
    assert dev_d <= max(proto.FACTOR * dev_p, proto.FLOOR)
    # stage 1 of fb_lss_dmargins is these bits: smin and its frequency from them, by the kernel's own expression
    sel = _call(fb, world, proto.W_CLOSED, every=False)[0]
    world.close()
    for i in list(range(13)) + [63, 64, 129]:
        s2 = [_fma_sq(1.0 + v.real, v.imag) for v in full[:, i]]
        k = int(np.argmin(s2))
        assert sel[8, i] == np.sqrt(s2[k]) and sel[9, i] == proto.W_CLOSED[k], i


# ---- 4, 5. position independence; unequal work inside one wave ------------------------------------------------------------------------------------------
def test_unequal_work_inside_one_wave_and_position_independence(fb, capsys):
    named = proto.work_systems()
    cont, w, Ts = [s for _, s in named], proto.W_WORK, proto.TS_WORK
    world = _held(fb, cont, Ts)
    big = _call(fb, world, w)
    again = _call(fb, world, w)
    sampled = _systems(world)
    world.close()
    assert same(again, big) and (big[3] == 0).all()
    counts = [tuple(big[1][:, i]) for i in range(len(named))]
    assert {sum(c) for c in counts[:8]} >= {0, 1, 2, 3}          # 0, 1, 2 and 3 crossings in the first group-of-8 wave
    for i, s in enumerate(sampled):          # the counts are the exact side's, for all 130
        assert counts[i] == tuple(proto.exact(*s, w, Ts)[0][1]), (i, named[i][0])
    _hold(f"c2d of 0 to 3 crossings in nx = {mp.NX_WORK}", take(big, slice(0, 10)), [_ref(s, w, Ts) for s in sampled[:10]], capsys)
    for i in list(range(10)) + [63, 64, 129]:          # each system alone
        assert same(_run_held(fb, [cont[i]], w, Ts), take(big, [i])), i
    assert same(take(_run_held(fb, cont[::-1], w, Ts), np.arange(len(cont))[::-1]), big)          # other places, other neighbours
    for n in (3, 9, 63):
        assert same(_run_held(fb, cont[:n], w, Ts), take(big, np.arange(n))), n


# ---- 6. chunk edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [65, 66, 130])
def test_crossings_in_the_first_and_the_last_interval(fb, nw, capsys):
    for K in proto.K_DELAY:
        s, w = proto.delay_integrator(K), proto.edge_grid(K, nw)
        out = _run(fb, [s] * 3, w)
        assert (out[3] == 0).all() and (out[1] == 1).all()
        assert (out[2][0, 0] > w[-2]).all() and (out[2][3, 0] < w[1]).all()
        _hold(f"{nw} frequencies, K = {K:g}", out, [_ref(s, w)] * 3, capsys)


# ---- 7. more crossings than are kept --------------------------------------------------------------------------------------------------------------------
def test_more_than_kmax_crossings(fb, capsys):
    rng = np.random.default_rng(3)
    s, other = proto.modes(), mp.embed(proto.cube(4.0), 12, rng)
    w, Ts = proto.W_MODES, proto.TS_MODES
    world = _held(fb, [s, other, s], Ts)
    sel, counts, allv, status = out = _call(fb, world, w)
    sampled = _systems(world)
    world.close()
    assert status.tolist() == [proto.TRUNCATED, 0, proto.TRUNCATED] and counts[:, 0].tolist() == [0, proto.KMAX] and counts[:, 1].tolist() == [1, 1]
    assert (np.diff(allv[3, :, 0]) > 0.0).all() and np.isfinite(allv[3:, :, 0]).all() and np.isnan(allv[:3, :, 0]).all()
    _hold("c2d of six lightly damped modes", out, [_ref(x, w, Ts) for x in sampled], capsys)


# ---- 8. the gain ------------------------------------------------------------------------------------------------------------------------------------------
def test_gain(fb, capsys):
    s, w = proto.closed_systems(9)[1][0], proto.W_CLOSED
    one, k = _run(fb, [s], w), _run(fb, [s], w, gain=0.6)
    r6, r1 = _ref(s, w, TS, 0.6), _ref(s, w)
    _hold("gain 0.6", k, [r6], capsys)
    bound = max(proto.FACTOR * (r6[0] + r1[0]), proto.FLOOR)
    assert abs(k[0][0, 0] / (one[0][0, 0] / 0.6) - 1.0) <= bound and abs(k[0][1, 0] / one[0][1, 0] - 1.0) <= bound          # gm scales as 1 / gain
    gains = np.array([1.0, 0.6, 2.0, 0.3, 1.5])
    batch = _run(fb, [s] * 5, w, gain=gains)
    for i, g in enumerate(gains):
        assert same(_run(fb, [s], w, gain=g), take(batch, [i])), g
    assert same(take(batch, [0]), one)          # a NULL gain is ones


# ---- 9. bad inputs among healthy neighbours ---------------------------------------------------------------------------------------------------------------
def test_bad_inputs_among_healthy_neighbours(fb):
    w = proto.W_CLOSED[::2]
    healthy = [proto.delay_integrator(0.2 + 0.08 * i) for i in range(9)]
    clean = _run(fb, healthy, w)
    assert (clean[3] == 0).all() and (clean[1] == 1).all()
    bad = list(healthy)
    P = healthy[2][0].copy(); P[1, 0] = np.nan
    bad[2] = (P,) + healthy[2][1:]
    bad[6] = (healthy[6][0], 1e308 * healthy[6][1], 1e308 * healthy[6][2], 0.0)          # L overflows
    gains = np.ones(9); gains[4] = np.nan
    world = _given(fb, bad, TS)
    world.step(7)
    world.sync()
    snap = lambda: (world.x, world.u, *clock(fb, world), world.status, *world.model(), *world.model_cd(), world.params.dt, world.Ts)
    before = snap()
    sel, counts, allv, status = _call(fb, world, w, gains)
    fr = fb.dfreqresp(world, IU, IY, w)
    after = snap()
    world.close()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    assert status.tolist() == [0, 0, proto.NOT_FINITE, 0, proto.NOT_FINITE, 0, proto.SINGULAR, 0, 0]
    for i in (2, 4, 6):
        assert np.isnan(sel[:, i]).all() and np.isnan(allv[:, :, i]).all() and (counts[:, i] == 0).all()
    assert np.isnan(fr[:, [2, 6]]).all() and np.isfinite(fr[:, [0, 1, 3, 4, 5, 7, 8]]).all()
    ok = [0, 1, 3, 5, 7, 8]
    assert same(take((sel, counts, allv, status), ok), take(clean, ok))


# ---- 10. fb_lss_set_sampled ---------------------------------------------------------------------------------------------------------------------------------
def test_a_world_given_as_phi_gamma_is_the_c2d_world(fb):
    rng = np.random.default_rng(21)
    n, nx, Ts = 9, 6, 0.05
    cont = [mp.embed(proto.cube(K), nx, rng) for K in (2.0, 4.0, 7.0) * 3]
    lss = _lss(fb, cont)
    lss.x0 = np.zeros_like(lss.x0)          # x0 = 0: one step from the design point returns delta itself
    src = fb.LinearWorld(lss)
    a = fb.c2d(src, Ts).world
    src.close()
    Phi, Gam = a.model()
    Cm, D = a.model_cd()
    u0 = a.u.T.copy()
    a.f_ode()
    y0 = a.y.T.copy()
    a.step(1)
    a.sync()
    delta = a.x.T.copy()
    a.set_state(np.zeros((nx, n)))
    given = fb.LinearizedSS(xdot0=delta, x0=np.zeros((n, nx)), u0=u0, y0=y0, A=Phi, B=Gam, C=Cm, D=D, x_labels=a.x_labels, u_labels=a.u_labels,
                            y_labels=a.y_labels)
    b = fb.LinearWorld(given, Ts=Ts)
    assert b.Ts == Ts and b.params.dt == Ts and clock(fb, b) == (0.0, 0)
    assert all(bits(p, q) for p, q in zip(a.model() + a.model_cd(), b.model() + b.model_cd()))
    u = u0.T + rng.standard_normal((2, n))
    for spl in (1, 7, 50):
        for wd in (a, b):
            wd.set_state(np.zeros((nx, n)))
            wd.u = u
            wd.step(50, steps_per_launch=spl)
            wd.sync()
        assert bits(a.x, b.x) and clock(fb, a) == clock(fb, b) and np.isfinite(a.x).all() and np.abs(a.x).max() > 0.0, spl
        a.f_ode(); b.f_ode()
        assert bits(a.y, b.y)
    ia, ib = (fb.stepinfo(wd, [(IU, IY), (0, 0)], 2.0) for wd in (a, b))
    for f in ("y0", "yf", "stepsize", "peak", "peaktime", "overshoot", "undershoot", "settlingtime", "risetime", "status"):
        assert np.array_equal(getattr(ia, f), getattr(ib, f), equal_nan=True), f
    w = proto.w_zoh(Ts)
    assert same(_call(fb, a, w), _call(fb, b, w)) and np.array_equal(fb.dpoles(a).poles, fb.dpoles(b).poles)
    # a sampled handle under the continuous verbs, like a c2d result
    for verb in (lambda: fb.poles(b), lambda: fb.margins(b, u=IU, y=IY), lambda: fb.pidopt.freqresp(b, IU, IY, w), lambda: fb.c2d(b, Ts)):
        with pytest.raises(fb.FlightBatchError, match="sampled model"):
            verb()
    a.close(); b.close()


def test_set_sampled_refusals_and_what_it_leaves(fb):
    n = 3
    lss = _lss(fb, [proto.delay_integrator(0.5)] * n)
    world = fb.LinearWorld(lss)
    world.step(3, dt=1e-3)
    world.sync()
    x, u, ck = world.x, world.u, clock(fb, world)
    for Ts in (0.0, -0.02, np.inf, np.nan):
        assert fb.lib.fb_lss_set_sampled(world._h, Ts) != 0
        err = fb.lib.fb_last_error()
        assert b"fb_lss_set_sampled" in err and b"must be positive and finite" in err and world.Ts == 0.0, err
    assert fb.lib.fb_lss_set_sampled(world._h, 0.02) == 0
    assert world.Ts == 0.02 and world.params.dt == 0.02 and bits(world.x, x) and bits(world.u, u) and clock(fb, world) == ck
    assert fb.lib.fb_lss_set_sampled(world._h, 0.02) != 0 and b"already a sampled model" in fb.lib.fb_last_error()
    world.close()
    assert fb.lib.fb_lss_set_sampled(None, 0.02) != 0 and b"fb_lss_set_sampled: null handle" in fb.lib.fb_last_error()
    r = fb.Robot2DWorld(n)
    assert fb.lib.fb_lss_set_sampled(r._h, 0.02) != 0 and b"not a LinearizedSS handle" in fb.lib.fb_last_error()
    r.close()
    hh = C.c_void_p()
    assert fb.lib.fb_lss_create(2, 2, 2, n, 0, C.byref(hh)) == 0
    assert fb.lib.fb_lss_set_sampled(hh, 0.02) != 0 and b"no model yet" in fb.lib.fb_last_error()
    fb.lib.fb_destroy(hh)
    with pytest.raises(fb.FlightBatchError, match="must be positive and finite"):
        fb.LinearWorld(lss, Ts=0.0)


# ---- 11. fb_lss_dpoles ------------------------------------------------------------------------------------------------------------------------------------------
FLOOR_P, MARGIN_P = 1e-11, 10.0          # the rule of tests/test_gpu_poles.py


@pytest.mark.parametrize("nx", [2, 8, 9, 16, 17, 32])
def test_dpoles_against_lapack(fb, nx, capsys):
    n = 21
    A = np.asarray(pp.systems(nx, n))
    lam_p = pp.poles_batch(A)[0]
    mu = np.array([np.linalg.eigvals(a) for a in A])
    model = fb.design_model(A, np.ones((n, nx, 1)))
    cont, world = fb.LinearWorld(model), fb.LinearWorld(model, Ts=0.02)
    res, ref = fb.dpoles(world), fb.poles(cont)
    cont.close(); world.close()
    d, p = pp.batch_dev(res.poles, mu), pp.batch_dev(lam_p, mu)
    with capsys.disabled():
        print(f"\n[fb_lss_dpoles vs LAPACK] nx {nx:2d} x {n}: {d:.2e} (prototype {p:.2e})", end="")
    assert (res.status == 0).all() and d <= max(MARGIN_P * p, FLOOR_P)
    assert np.array_equal(res.poles, ref.poles) and np.array_equal(res.iters, ref.iters)          # the same kernel on the same matrix
    for i in range(n):
        assert pp.sort_rule_holds(res.poles[i]), i
    s = np.log(res.poles) / 0.02          # Python's reading against log on the host
    assert np.allclose(res.s, s, rtol=1e-15, atol=0.0) and np.array_equal(res.wn, np.abs(res.s))
    assert np.allclose(res.zeta, -np.cos(np.angle(s)), rtol=0.0, atol=1e-15) and np.allclose(res.tau, -1.0 / s.real, rtol=1e-14, atol=0.0)
    assert np.array_equal(res.stable, np.abs(res.poles).max(axis=1) < 1.0)


def _designed(fb, world, capsys, label):
    """dlqr(closed=True) -> dpoles on a sampled world: every |z| < 1, and the poles are the eigenvalues of Φ - Γ K from the returned K"""
    nx, nu = world.nx, world.nu
    res = fb.dlqr(world, np.eye(nx), np.eye(nu), closed=True)
    assert (res.status == 0).all()
    Phi, Gam = world.model()
    Pc = res.world.model()[0]
    assert np.abs(Pc - (Phi - Gam @ res.K)).max() <= 1e-12 * max(1.0, np.abs(Phi).max())
    got = fb.dpoles(res.world)
    res.world.close()
    mu = np.array([np.linalg.eigvals(a) for a in Phi - Gam @ res.K])
    lam_p = pp.poles_batch(Pc)[0]
    d, p = pp.batch_dev(got.poles, mu), pp.batch_dev(lam_p, mu)
    with capsys.disabled():
        print(f"\n[c2d -> dlqr -> dpoles] {label}: {d:.2e} of eig(Φ - Γ K) (prototype {p:.2e}); max |z| {np.abs(got.poles).max():.4f}", end="")
    assert (got.status == 0).all() and got.stable.all() and (np.abs(got.poles) < 1.0).all()
    assert d <= max(MARGIN_P * p, FLOOR_P)
    return got


def test_the_design_chain_ends_in_poles_inside_the_circle(fb, capsys):
    rng = np.random.default_rng(31)
    n, nx, nu, Ts = 9, 6, 2, 0.05
    A = rng.standard_normal((n, nx, nx)) + 0.5 * np.eye(nx)          # unstable plants
    B = rng.standard_normal((n, nx, nu))
    src = fb.LinearWorld(fb.design_model(A, B))
    zoh = fb.c2d(src, Ts).world
    src.close()
    assert not fb.dpoles(zoh).stable.any()
    _designed(fb, zoh, capsys, "unstable plants, nx = 6")
    # the same plants with one sample of computational delay: the input the plant sees is the last sample's — Φ gets nu eigenvalues at 0
    Phi, Gam = zoh.model()
    zoh.close()
    Pd, Gd = np.zeros((n, nx + nu, nx + nu)), np.zeros((n, nx + nu, nu))
    Pd[:, :nx, :nx], Pd[:, :nx, nx:], Gd[:, nx:, :] = Phi, Gam, np.eye(nu)
    delayed = fb.LinearWorld(fb.design_model(Pd, Gd), Ts=Ts)
    open_poles = fb.dpoles(delayed)
    assert (open_poles.status == 0).all() and (np.abs(open_poles.poles[:, :nu]) <= 1e-12).all()
    _designed(fb, delayed, capsys, "with a sample of delay, nx = 8")
    delayed.close()


def test_a_pole_at_zero_reads_as_damp_reads_it(fb):
    world = _given(fb, [proto.delay_integrator(0.5)], TS)
    res = fb.dpoles(world)
    world.close()
    assert res.status[0] == 0 and np.array_equal(res.poles[0], [0.0, 1.0])          # Φ = [[1, 0], [1, 0]]: 0 and the integrator's 1
    assert res.wn[0, 0] == np.inf and res.zeta[0, 0] == 1.0 and res.tau[0, 0] == 0.0 and not res.stable[0]
    assert res.wn[0, 1] == 0.0          # z = 1 is s = 0
    text = fb.ddampreport(res, 0)
    rows = text.split("\n")[3:]
    cells = [[c.strip() for c in row.split("|")[1:-1]] for row in rows]
    assert len(rows) == 2 and cells[0][0] == "+1" and cells[1][0] in ("+0", "-0") and cells[1][1:] == ["1", "Inf", "Inf", "0"]      # sorted by natural frequency


# ---- 12. margins and stability agree -------------------------------------------------------------------------------------------------------------------------------
def test_margins_and_stability_agree(fb):
    Ks = proto.K_STABILITY
    loops = [proto.delay_integrator(K) for K in Ks]
    world = _given(fb, loops, TS)
    gm = _call(fb, world, proto.W_CLOSED)[0][0]
    world.close()
    closed = np.array([P - np.outer(g, c) for P, g, c, _ in loops])          # 1 + L = 0: Φ - γ c
    cw = fb.LinearWorld(fb.design_model(closed, np.ones((len(Ks), 2, 1))), Ts=TS)
    stable = fb.dpoles(cw).stable
    cw.close()
    assert (gm > 1.0).tolist() == stable.tolist() == [K < 1.0 for K in Ks]


# ---- 13. refusals launch nothing -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n, grid = 5, proto.W_CLOSED[:17].copy()
    world = _given(fb, [proto.delay_integrator(0.5)] * n, TS)
    sel, counts, status, allv = np.empty((10, n)), np.empty((2, n), dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((6, proto.KMAX, n))
    re_, im_, pr, pim, it = np.empty((1025, n)), np.empty((1025, n)), np.empty(2 * n), np.empty(2 * n), np.empty(n, dtype=np.int32)

    def dmargins(h, iu=IU, iy=IY, w=grid, nw=None, sel=sel, counts=counts, status=status):
        return fb.lib.fb_lss_dmargins(h, iu, iy, pd(w), (0 if w is None else w.size) if nw is None else nw, None, pd(sel), pi(counts), pd(allv), pi(status))

    def dfreqresp(h, iu=IU, iy=IY, w=grid, nw=None, re=re_, im=im_, **_):
        return fb.lib.fb_lss_dfreqresp(h, iu, iy, pd(w), (0 if w is None else w.size) if nw is None else nw, pd(re), pd(im))

    def dpoles(h, **_):
        return fb.lib.fb_lss_dpoles(h, pd(pr), pd(pim), pi(it), pi(status))

    verbs = {b"fb_lss_dmargins": dmargins, b"fb_lss_dfreqresp": dfreqresp, b"fb_lss_dpoles": dpoles}

    def refused(name, h, cause, timed=True, **kw):
        if timed:
            assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        rc = verbs[name](h, **kw)
        err = fb.lib.fb_last_error()
        assert rc != 0 and cause in err and name in err, (name, cause, err)
        assert not timed or _launches(fb, h) == 0, err

    r = fb.Robot2DWorld(n)
    hh = C.c_void_p()
    assert fb.lib.fb_lss_create(2, 2, 2, n, 0, C.byref(hh)) == 0
    cont = fb.LinearWorld(_lss(fb, [proto.cube(4.0)] * n))
    for name in verbs:
        refused(name, None, b"null handle", timed=False)
        refused(name, r._h, b"not a LinearizedSS handle", timed=False)          # (a Robot2D handle keeps no per-launch stamps)
        refused(name, hh, b"no model yet")
        refused(name, cont._h, b"a discrete-time verb on a continuous model")
    r.close(); cont.close()
    fb.lib.fb_destroy(hh)
    h = world._h
    above = grid.copy(); above[-1] = np.nextafter(np.pi / TS, np.inf) * 1.0000001
    for name in (b"fb_lss_dmargins", b"fb_lss_dfreqresp"):
        refused(name, h, b"iu = 2 is outside", iu=2)
        refused(name, h, b"iu = -1 is outside", iu=-1)
        refused(name, h, b"iy = 2 is outside", iy=2)
        refused(name, h, b"the frequency grid w is required", w=None, nw=17)
        refused(name, h, b"nw = 1025,", w=np.linspace(1.0, 100.0, 1025))
        refused(name, h, b"nw = 0,", nw=0)
        for k, v in ((3, 0.0), (3, -1.0), (3, np.inf), (3, np.nan)):
            g = grid.copy(); g[k] = v
            refused(name, h, b"must be positive and finite", w=g)
        refused(name, h, b"above the Nyquist frequency pi/Ts", w=above)
    refused(b"fb_lss_dfreqresp", h, b"re and im are required", re=None)
    refused(b"fb_lss_dfreqresp", h, b"re and im are required", im=None)
    refused(b"fb_lss_dmargins", h, b"sel, counts and status are required", sel=None)
    refused(b"fb_lss_dmargins", h, b"sel, counts and status are required", counts=None)
    refused(b"fb_lss_dmargins", h, b"sel, counts and status are required", status=None)
    refused(b"fb_lss_dmargins", h, b"nw = 1,", nw=1)
    g = grid.copy(); g[5] = g[4]
    refused(b"fb_lss_dmargins", h, b"must strictly increase", w=g)
    refused(b"fb_lss_dmargins", h, b"must strictly increase", w=grid[::-1].copy())
    nyq = np.array([1.0, np.pi / TS])          # the Nyquist frequency itself is inside the grid's range
    if nyq[1] * TS <= np.pi:
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        assert dfreqresp(h, w=nyq) == 0 and _launches(fb, h) == 1
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert dmargins(h) == 0 and _launches(fb, h) == 2          # the grid response in one slice, then the margins
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert dfreqresp(h) == 0 and _launches(fb, h) == 1
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert dpoles(h) == 0 and _launches(fb, h) == 1
    with pytest.raises(ValueError, match="2 to 1024"):
        fb.dmargins(world, w=grid[:1])
    res = fb.dmargins(world, u=IU, y=IY)          # the default grid reaches the Nyquist frequency and passes the library's check
    assert res.ok.all() and (res.npc == 1).all() and (res.ngc == 1).all()
    assert abs(res.gm[0] - 2.0) <= 1e-12 and abs(res.wpc[0] * TS / (np.pi / 3.0) - 1.0) <= 1e-12
    world.close()
    # N nw above 2^31 - 1: 2^21 systems of one state on 1024 frequencies
    big_n = 1 << 21
    z, o = np.zeros((big_n, 1)), np.ones((big_n, 1, 1))
    big = fb.LinearWorld(fb.LinearizedSS(xdot0=z, x0=z, u0=z, y0=z, A=0.5 * o, B=o, C=o, D=0.0 * o, x_labels=("x",), u_labels=("u",), y_labels=("y",)),
                         Ts=TS)
    assert fb.lib.fb_timing_begin_per_launch(big._h, 8) == 0
    rc = fb.lib.fb_lss_dmargins(big._h, 0, 0, pd(np.linspace(1.0, 100.0, 1024)), 1024, None, pd(sel), pi(counts), None, pi(status))
    err = fb.lib.fb_last_error()
    assert rc != 0 and b"exceed the 2^31 - 1 pairs" in err and _launches(fb, big._h) == 0, err
    big.close()


# ---- 14. the example ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sampled_margins.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GM" in r.stdout and "PM" in r.stdout and "delay" in r.stdout
