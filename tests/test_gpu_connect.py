"""fb_lss_connect (flightbatch.connect): two batches of linear models connected through static gains on the device, pinned by

  1. the longdouble restatement (tests/connect_prototype.py) on twelve shapes x N in {1, 63, 130}: every P of the kernel at its smallest and
     its largest size, plant and compensator in every handle group size;
  2. position independence and reproducibility, bit for bit, and the sources left as they were;
  3. the new handle as a full citizen: the same bits as a handle loaded from its (A, B, C, D), stepping and f_ode, under both exchanges;
  4. an ill-posed and a non-finite system flagged in place among healthy ones;
  5. the refusals of the C ABI on a live device;
  6. the Robot2D notebook's stored tables, the q2e plants and the pitch-rate loop of the 28 design nodes, end to end on the device.

The bound of 1 and 6 is the family's rule: the device differs from the float64 restatement in FMA contraction, in the term a sum starts from
and in <= 1-ulp division only, so its deviation from the longdouble side may be ten times the prototype's over the same systems, with 1e-13
as the floor (about 40 times the worst prototype deviation tests/test_connect_host.py measures; any indexing error is of order 1). A
deviation is max|got - want| over a block divided by the block's largest |want|, per system, the worst over the batch. Measured on one
MI355X: at most 9.6e-16 on every block of every shape but the 1 x 1 block D' of 8/1/2/1/8/1/9/1/1 (4.99e-15, the prototype 4.79e-15: a
cancelling sum); the figures are in docs/design/linearize.md, "Closing loops on the device"."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import connect_prototype as proto
import pid_prototype
import poles_prototype
import reference_fixtures as rf
import timeresp_prototype
from support import LSS_EXCHANGES, clock, exchange, gains_from_h5

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-13, 10.0
BLOCKS = ("A'", "B'", "C'", "D'")
MID = (15, 1, 4, 1, 33, 1, 16, 4, 34)
pi32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
same = lambda a, b: np.array_equal(a, b, equal_nan=True)


def _lss(fb, side, tag, seed):
    """a side (A, B, C, D) [n, ., .] as a LinearizedSS whose xdot0, x0, u0, y0 are random numbers (they play no part)"""
    A, B, Cm, D = side
    n, nx, nu, ny = A.shape[0], A.shape[1], B.shape[2], Cm.shape[1]
    rng = np.random.default_rng(seed)
    return fb.LinearizedSS(xdot0=rng.standard_normal((n, nx)), x0=rng.standard_normal((n, nx)), u0=rng.standard_normal((n, nu)),
                           y0=rng.standard_normal((n, ny)), A=A, B=B, C=Cm, D=D, x_labels=tuple(f"x{tag}{k}" for k in range(nx)),
                           u_labels=tuple(f"u{tag}{k}" for k in range(nu)), y_labels=tuple(f"y{tag}{k}" for k in range(ny)))


def _take(side, keep):
    return None if side is None else tuple(np.ascontiguousarray(m[keep]) for m in side)


def _worlds(fb, P, Cc):
    return fb.LinearWorld(_lss(fb, P, "p", 1)), (fb.LinearWorld(_lss(fb, Cc, "c", 2)) if Cc is not None else None)


def _read(res):
    w = res.world
    out = w.model() + w.model_cd() + (res.status.copy(),)
    w.close()
    return out


def _connect(fb, cs, keep=slice(None), batch_wide=None):
    """(A', B', C', D', status) of the systems `keep` of a case; batch_wide = i: system i's F and G for the whole batch, as [nv, .] matrices"""
    P, Cc, jz, F, G, iz = cs
    pw, cw = _worlds(fb, _take(P, keep), _take(Cc, keep))
    Fk, Gk = (F[keep], G[keep]) if batch_wide is None else (F[batch_wide], G[batch_wide])
    res = fb.connect(pw, cw, feedback=Fk, inputs=Gk, reads=jz, outputs=iz)
    assert res.world.n == pw.n and (res.world.nx, res.world.nu, res.world.ny) == (P[0].shape[1] + (Cc[0].shape[1] if Cc else 0), G.shape[2], len(iz))
    out = _read(res)
    pw.close()
    if cw is not None:
        cw.close()
    return out


def _hold(label, got, long, f64, capsys):
    dev = [float(proto.block_dev(g, l).max()) for g, l in zip(got, long)]
    pro = [float(proto.block_dev(f, l).max()) for f, l in zip(f64, long)]
    with capsys.disabled():
        print(f"\n[{label}] device (prototype) vs longdouble: " + "  ".join(f"{b} {d:.2e} ({p:.2e})" for b, d, p in zip(BLOCKS, dev, pro)), end="")
    for b, d, p in zip(BLOCKS, dev, pro):
        assert d <= max(MARGIN * p, FLOOR), (label, b, d, p)


# ---- 1. accuracy -----------------------------------------------------------------------------------------------------------------------------------
def test_the_shapes_cover_every_group_size():
    assert {proto.group(s[0] + s[1], s[2] + s[3]) for s in proto.SHAPES} == {8, 16, 32}
    assert {proto.handle_group(s[0]) for s in proto.SHAPES} == {4, 8, 16, 32} == {proto.handle_group(s[1]) for s in proto.SHAPES if s[1]}
    for P in (8, 16, 32):      # each P at the smallest and at the largest size that selects it
        sizes = {max(s[0] + s[1], s[2] + s[3]) for s in proto.SHAPES if proto.group(s[0] + s[1], s[2] + s[3]) == P}
        assert {P // 2 + 1 if P > 8 else 1, P} <= sizes, (P, sizes)


@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("shape", proto.SHAPES, ids=lambda s: "/".join(map(str, s)))
def test_against_the_longdouble_side(fb, shape, n, capsys):
    cs, f64, long = proto.sides(shape)
    got = _connect(fb, cs, slice(0, n))
    assert (got[4] == 0).all() and (f64[4] == 0).all()
    _hold(f"fb_lss_connect {'/'.join(map(str, shape))} N {n}", got[:4], [m[:n] for m in long[:4]], [m[:n] for m in f64[:4]], capsys)


# ---- 2. bit for bit --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid(fb):
    out = _connect(fb, proto.sides(MID)[0])
    for a in out:
        a.setflags(write=False)
    return out


def test_a_second_call_and_the_batch_in_another_order(fb):
    cs = proto.sides(MID)[0]
    full = _mid(fb)
    again = _connect(fb, cs)
    assert all(same(a, b) for a, b in zip(full, again))
    rev = _connect(fb, cs, slice(None, None, -1))
    assert all(same(a, b[::-1]) for a, b in zip(full, rev))
    keep = np.array([129, 3, 64, 63, 0, 77, 12])
    sub = _connect(fb, cs, keep)
    assert all(same(a[keep], b) for a, b in zip(full, sub))
    for n in (1, 63):
        head = _connect(fb, cs, slice(0, n))
        assert all(same(a[:n], b) for a, b in zip(full, head))


def test_batch_wide_gains_are_the_replicated_ones(fb):
    P, Cc, jz, F, G, iz = proto.sides(MID)[0]
    n = 63
    rep = (_take(P, slice(0, n)), _take(Cc, slice(0, n)), jz, np.repeat(F[5:6], n, axis=0), np.repeat(G[5:6], n, axis=0), iz)
    per = _connect(fb, rep)
    wide = _connect(fb, (P, Cc, jz, F, G, iz), slice(0, n), batch_wide=5)
    assert (per[4] == 0).all() and all(same(a, b) for a, b in zip(per, wide))


def test_the_sources_are_left_as_they_were(fb):
    P, Cc, jz, F, G, iz = proto.sides(MID)[0]
    pw, cw = _worlds(fb, P, Cc)
    rng = np.random.default_rng(8)
    for w in (pw, cw):
        w.set_params(dt=0.004)
        w.u = rng.standard_normal((w.nu, w.n))
    pw.log_configure(every=2, capacity=8, y=[0, 1], x=[0])
    pw.step(7)
    pw.sync()

    def snapshot(w):
        t, data = w.log_read() if w is pw else (np.zeros(0), np.zeros(0))
        return (w.x, w.u, w.status, np.array(clock(fb, w)), t, data) + w.model() + w.model_cd()
    before = [snapshot(w) for w in (pw, cw)]
    res = fb.connect(pw, cw, feedback=F, inputs=G, reads=jz, outputs=iz)
    after = [snapshot(w) for w in (pw, cw)]
    for b, a in zip(before, after):
        assert all(same(x, y) for x, y in zip(b, a))
    assert clock(fb, pw) == (pytest.approx(7 * 0.004), 7) and not before[0][2].any()      # (a linear model's status words stay 0)
    # the new handle: p's dt, at rest, clock at zero
    w = res.world
    assert clock(fb, w) == (0.0, 0) and not w.x.any() and not w.u.any() and (w.status == 0).all()
    w.step(1)
    w.sync()
    assert clock(fb, w) == (pytest.approx(0.004), 1)
    assert all(same(a, b) for a, b in zip(_read(res), _mid(fb)))
    pw.close(); cw.close()


# ---- 3. a full citizen -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xch", LSS_EXCHANGES)
def test_the_new_handle_is_an_ordinary_one(fb, xch):
    P, Cc, jz, F, G, iz = proto.sides((7, 1, 2, 1, 3, 1, 2, 2, 4))[0]
    with exchange(xch):
        pw, cw = _worlds(fb, P, Cc)
        res = fb.connect(pw, cw, feedback=F, inputs=G, reads=jz, outputs=iz)
        a = res.world
        A, B = a.model()
        Cm, D = a.model_cd()
        n = a.n
        z = np.zeros
        b = fb.LinearWorld(fb.LinearizedSS(xdot0=z((n, a.nx)), x0=z((n, a.nx)), u0=z((n, a.nu)), y0=z((n, a.ny)), A=A, B=B, C=Cm, D=D,
                                           x_labels=a.x_labels, u_labels=a.u_labels, y_labels=a.y_labels))
        assert a.exchange == b.exchange == xch
        assert a.x_labels == pw.x_labels + cw.x_labels and a.u_labels == ("w0", "w1") and a.y_labels == tuple((pw.y_labels + cw.y_labels)[k] for k in iz)
        rng = np.random.default_rng(11)
        x0, u = rng.standard_normal((a.nx, n)), rng.standard_normal((a.nu, n))
        outs = []
        for w in (a, b):
            w.set_state(x0)
            w.set_params(dt=0.003)
            w.u = u
            xd = np.empty((w.nx, n))
            w.f_ode(xd)
            y0 = w.y
            assert fb.lib.fb_set_steps_per_launch(w._h, 7) == 0
            w.step(50)
            w.sync()
            w.f_ode()
            outs.append((xd, y0, w.x, w.y, np.array(clock(fb, w))))
        assert all(same(p, q) for p, q in zip(*outs)) and np.isfinite(outs[0][2]).all() and outs[0][2].any()
        # and the design verbs take it
        assert fb.poles(a).status.shape == (n,) and same(fb.poles(a).poles, fb.poles(b).poles)
        for w in (a, b, pw, cw):
            w.close()


def test_state_feedback_is_closed_loop(fb, capsys):
    """flightbatch.lqr.closed_loop's A - B K, C - D K (C = I, D = 0 of a design model) and B K_fwd, by the accuracy rule"""
    rng = np.random.default_rng(17)
    n, nx, nu = 9, 6, 3
    m = fb.design_model(rng.standard_normal((n, nx, nx)), rng.standard_normal((n, nx, nu)))
    K, Kf = rng.standard_normal((n, nu, nx)), rng.standard_normal((nu, 2))
    cl = fb.closed_loop(m, K)
    w = fb.LinearWorld(m)
    for K_fwd, G, labels in ((None, np.eye(nu), w.u_labels), (Kf, Kf, ("w0", "w1"))):
        res = fb.state_feedback(w, K, K_fwd)
        assert res.ok.all() and res.world.u_labels == labels and res.world.x_labels == w.x_labels == res.world.y_labels
        got = _read(res)
        args = ((m.A, m.B, m.C, m.D), None, list(range(nx)), -K, G, None)
        pro, long = proto.connect_batch(*args), proto.connect_batch(*args, dtype=np.longdouble)
        assert np.array_equal(pro[0], cl.A) and np.array_equal(pro[2], cl.C) and (K_fwd is not None or np.array_equal(pro[1], cl.B))
        assert not got[3].any()      # D' = D K_fwd = 0: a block whose largest entry is 0 is held to equality
        _hold(f"state_feedback, K_fwd {'given' if K_fwd is not None else 'None'}", got[:3], long[:3], pro[:3], capsys)
    w.close()


# ---- 4. failures in place ------------------------------------------------------------------------------------------------------------------------------
def _robot2d_batch(n):
    lin = json.load(open(os.path.join(timeresp_prototype.GOLDEN, "robot2d_linearization.json"), encoding="utf-8"))
    rng = np.random.default_rng(13)
    side = tuple(np.repeat(np.array(lin[k])[None], n, axis=0) for k in "ABCD")
    side[0][:, :2, :3] *= 1.0 + 0.05 * rng.standard_normal((n, 2, 3))      # every system its own
    return side


def test_an_ill_posed_and_a_non_finite_system_among_healthy_ones(fb):
    n, bad, nanf = 65, 17, 40
    P = _robot2d_batch(n)
    integ = tuple(np.repeat(m[None], n, axis=0) for m in proto.integrator())
    g = gains_from_h5()
    # z = ω, v, θ, η, u_m, τ_m, ξ; the feedback also reads u_m, whose D is 1: gain 0.25 on the healthy systems, exactly 1 on one
    F = np.zeros((n, 2, 5))
    F[:, 0, :3] = -g[0:3]; F[:, 0, 3] = -1.0; F[:, 0, 4] = 0.25; F[:, 1, 1] = g[4]
    F[bad, 0, 4] = 1.0
    F[nanf, 1, 2] = np.nan
    G = np.repeat(np.array([[g[3]], [-g[4]]])[None], n, axis=0)
    cs = (P, integ, np.array([0, 1, 2, 6, 4], dtype=np.int32), F, G, np.arange(7, dtype=np.int32))
    got = _connect(fb, cs)
    expect = np.zeros(n, dtype=np.int32); expect[bad] = fb.K["FB_CONNECT_ILL_POSED"]; expect[nanf] = fb.K["FB_CONNECT_NOT_FINITE"]
    assert np.array_equal(got[4], expect), got[4]
    for m in got[:4]:
        assert np.isnan(m[bad]).all() and np.isnan(m[nanf]).all()
    healthy = np.flatnonzero(expect == 0)
    assert healthy.size == 63
    ref = _connect(fb, cs, healthy)
    assert (ref[4] == 0).all() and all(same(a[healthy], b) and np.isfinite(b).all() for a, b in zip(got[:4], ref[:4]))
    pro = proto.connect_batch(*cs)
    assert np.array_equal(pro[4], expect)
    # a non-finite entry of a source model that no row of jz or iz reads is one all the same
    P2 = tuple(m.copy() for m in P)
    P2[2][3, 5, 1] = np.inf
    got2 = _connect(fb, (P2, integ, cs[2], np.where(np.isnan(F), 0.0, F), G, np.array([0, 1], dtype=np.int32)))
    assert got2[4][3] == fb.K["FB_CONNECT_NOT_FINITE"] and got2[4][bad] == fb.K["FB_CONNECT_ILL_POSED"] and np.count_nonzero(got2[4]) == 2


def test_the_ill_posed_pid_pair_is_the_singular_one_of_pid_metrics(fb):
    """1 / (s + 1) - 0.5 with p = (2, 0, 0, 0.01): 1 + d (k_p + k_d / tau_f) = 0"""
    A, b, c, d = np.full((2, 1, 1), -1.0), np.ones((2, 1)), np.ones((2, 1)), np.array([-0.5, 0.0])
    p = np.array([[2.0, 0.0, 0.0, 0.01], [2.0, 0.0, 0.0, 0.01]])
    pw = fb.LinearWorld(pid_prototype.model(fb, A, b, c, d))
    cw = fb.pid_world(p)
    res = fb.unity_feedback(pw, cw, "u", "y")
    met = fb.pid_metrics(pw, p[:, None, :], settings=fb.Settings(t_sim=1.0, dt=1e-2, w=pid_prototype.W7))
    assert list(res.status) == [fb.K["FB_CONNECT_ILL_POSED"], 0] and list(met.status[:, 0]) == [fb.K["FB_PID_SINGULAR"], 0]
    assert list(res.ok) == [False, True] and res.world.u_labels == ("y_ref",) and res.world.y_labels == ("y", "u")
    A1, B1 = res.world.model()
    assert np.isnan(A1[0]).all() and np.isfinite(A1[1]).all()
    for w in (res.world, pw, cw):
        w.close()


# ---- 5. refusals on a live device ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 5
    mk = lambda nx, nu, ny, nn=n, seed=0: fb.LinearWorld(_lss(fb, tuple(np.random.default_rng(seed).standard_normal(s) for s in
                                                                      ((nn, nx, nx), (nn, nx, nu), (nn, ny, nx), (nn, ny, nu))), "p", 3))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def call(p, c=None, jz=(0,), nf=None, F=True, G=True, nw=1, iz=(0,), ny=None, out=True, timed=True):
        if timed:
            assert fb.lib.fb_timing_begin_per_launch(p, 8) == 0
        cj = None if jz is None else np.array(jz, dtype=np.int32)
        ci = None if iz is None else np.array(iz, dtype=np.int32)
        buf = np.zeros(16 * 32 * 8)
        h = C.c_void_p(1)
        rc = fb.lib.fb_lss_connect(p, c, pi32(cj), len(jz) if nf is None else nf, pd(buf) if F else None, 0, pd(buf) if G else None, 0, nw,
                                   pi32(ci), (len(iz) if iz is not None else 0) if ny is None else ny, None, C.byref(h) if out else None)
        err = fb.lib.fb_last_error()
        if rc == 0:
            fb.lib.fb_destroy(h)
        else:
            assert not out or not h.value       # no handle behind a refusal
        return rc, err, (launches(p) if timed else 0)

    def refused(p, cause, **kw):
        rc, err, nl = call(p, **kw)
        assert rc != 0 and b"fb_lss_connect" in err and cause in err and nl == 0, (cause, err, nl)

    refused(None, b"null handle", timed=False)
    r = fb.Robot2DWorld(n)
    refused(r._h, b"the plant is not a LinearizedSS handle", timed=False)      # (a Robot2D handle keeps no per-launch stamps)
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.connect(r, feedback=np.zeros((1, 1)), inputs=np.ones((1, 1)), reads=[0])
    w = mk(3, 2, 4)
    refused(w._h, b"the compensator is not a LinearizedSS handle", c=r._h)
    r.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 3, n, 0, C.byref(h)) == 0
    refused(h, b"the plant has no model yet")
    refused(w._h, b"the compensator has no model yet", c=h)
    fb.lib.fb_destroy(h)
    other = mk(2, 1, 1, nn=n + 1)
    refused(w._h, b"the compensator has N = 6 systems, the plant N = 5", c=other._h)
    other.close()
    big, big2 = mk(20, 8, 64), mk(13, 8, 64)
    refused(big._h, b"nx_p + nx_c = 33", c=big2._h)
    # nv > FB_CONNECT_NV_MAX and nz > FB_CONNECT_NZ_MAX cannot be built from two handles (nu <= 8 and ny <= 64 each): 16 and 128 are reached
    c9, c6 = mk(2, 8, 64, seed=1), mk(1, 1, 2, seed=5)
    rc, err, nl = call(big._h, c=c9._h)
    assert rc == 0 and nl == 1, err
    refused(w._h, b"nf = 0", jz=(), nf=0)
    refused(w._h, b"nf = 33", jz=(0,) * 33)
    refused(w._h, b"nw = 0", nw=0)
    refused(w._h, b"nw = 9", nw=9)
    refused(w._h, b"ny = 0", iz=(), ny=0)
    refused(w._h, b"ny = 65", iz=(0,) * 65)
    refused(w._h, b"jz[1] = 4 is outside [0, 4)", jz=(0, 4))
    refused(w._h, b"jz[0] = -1 is outside", jz=(-1,))
    refused(w._h, b"iz[0] = 6 is outside [0, 6)", c=c6._h, iz=(6,))
    refused(w._h, b"F, G and jz are required", F=False)
    refused(w._h, b"F, G and jz are required", G=False)
    refused(w._h, b"F, G and jz are required", jz=None, nf=1)
    refused(w._h, b"out is null", out=False)
    refused(big._h, b"iz is NULL", c=c9._h, iz=None)
    rc, err, nl = call(w._h, iz=None)          # every row of z
    assert rc == 0 and nl == 1, err
    with pytest.raises(KeyError, match="not an output label"):
        fb.connect(w, feedback=np.zeros((2, 1)), inputs=np.ones((2, 1)), reads=["nope"])
    with pytest.raises(ValueError, match="feedback must be"):
        fb.connect(w, feedback=np.zeros((3, 1)), inputs=np.ones((2, 1)), reads=[0])
    for x in (w, big, big2, c9, c6):
        x.close()


# ---- 6. end to end against what the reference stores ---------------------------------------------------------------------------------------------------
def test_the_notebooks_tables_from_linearize_through_connect(fb, capsys):
    w = fb.Robot2DWorld(3)
    fb.linearize(w, None, scheme="forward")
    plant = fb.linear_world(w)
    w.close()
    g = gains_from_h5()
    K_x, K_fwd, K_int = g[0:3], g[3], g[4]
    integ = fb.integrator_world(3)
    F = np.array([[-K_x[0], -K_x[1], -K_x[2], -1.0], [0.0, K_int, 0.0, 0.0]])
    vel = fb.connect(plant, integ, feedback=F, inputs=np.array([[K_fwd], [-K_int]]), reads=["ω", "v", "θ", "ξ"], input_labels=("v_ref",))
    assert vel.ok.all() and vel.world.x_labels == ("ω", "v", "θ", "η", "ξ") and vel.world.y_labels == ("ω", "v", "θ", "η", "u_m", "τ_m", "ξ")
    pos = fb.connect(vel.world, feedback=np.array([[-0.6]]), inputs=np.array([[0.6]]), reads=["η"], input_labels=("η_ref",))
    assert pos.ok.all()
    # the loops are the host surgery's on the device's own A, B (which the prototype reproduces to the last bit; the device fuses its multiply-adds)
    A, B = plant.model()
    (Av, bv, cv, dv), (Ap, bp, ce, dp) = timeresp_prototype.notebook_loops(A[0], B[0])
    for res, (Al, bl) in ((vel, (Av, bv)), (pos, (Ap, bp))):
        Ad, Bd = res.world.model()
        for i in range(3):
            assert np.abs(Ad[i] - Al).max() <= FLOOR * np.abs(Al).max() and np.abs(Bd[i, :, 0] - bl).max() <= FLOOR * np.abs(bl).max()
    lam = fb.poles(vel.world)
    assert (lam.status == 0).all()
    poles_prototype.assert_matches_table(lam.poles[0], "velocity_loop")
    tables = timeresp_prototype.stored_tables()
    stable = {}
    for which, res, ch in (("velocity_loop", vel, ("v_ref", "v")), ("position_loop", pos, ("η_ref", "η"))):
        t = tables[which]
        assert (t["t_sim"], t["dt"]) == ((5.0, 0.0062) if which == "velocity_loop" else (10.0, 0.005))
        si = fb.stepinfo(res.world, [ch], t["t_sim"], dt=t["dt"])
        stable[which] = bool(fb.poles(res.world).stable[0])
        text = si.show(0, 0)
        with capsys.disabled():
            print(f"\n[connect, Robot2D {which}] " + "; ".join(" ".join(s.split()) for s in text.split("\n")), end="")
        assert si.ok.all()
        timeresp_prototype.assert_matches_table(text.split("\n"), which)
    assert stable == {"velocity_loop": False, "position_loop": True}
    for x in (plant, integ, vel.world, pos.world):
        x.close()


@functools.lru_cache(maxsize=None)
def _design_nodes_on_the_device(fb):
    """the te2te design model of the 28 nodes (a LinearWorld with C = I), K_fbk by fb_lqr, K_fwd on the host: tests/test_gpu_pid.py's chain, the
    design world kept"""
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
    lw = fb.LinearWorld(fb.design_model(Ar, Br, x_labels=xl, u_labels=ul))
    res = fb.lqr(lw, [float(qx.get(k, 0.0)) for k in xl], np.array(r, dtype=np.float64))
    assert (res.status == 0).all()
    Cz, Dz = rl._z_rows(xl, ul, zl)
    Kf = np.array([rl._k_fwd(Ar[k], Br[k], Cz, Dz, res.K[k]) for k in range(28)])
    return lw, Ar, Br, res.K, Kf, xl, ul


def _q2e_world(fb):
    """the q2e plants by connect: u = K_fwd[:, elevator_cmd] ξ - K_fbk x around the design world, the integrator's input the new input, q the output"""
    lw, Ar, Br, K, Kf, xl, ul = _design_nodes_on_the_device(fb)
    nx, nu = len(xl), len(ul)
    F = np.zeros((28, nu + 1, nx + 1))
    F[:, :nu, :nx] = -K
    F[:, :nu, nx] = Kf[:, :, ul.index("elevator_cmd")]
    G = np.zeros((nu + 1, 1)); G[nu, 0] = 1.0
    integ = fb.integrator_world(28)
    res = fb.connect(lw, integ, feedback=F, inputs=G, outputs=["q"], input_labels=("q_err",))
    integ.close()
    assert res.ok.all()
    return res.world, (Ar, Br, K, Kf, xl, ul, F, G)


def test_the_q2e_plants_by_connect(fb, capsys):
    pw, (Ar, Br, K, Kf, xl, ul, F, G) = _q2e_world(fb)
    assert (pw.nx, pw.nu, pw.ny) == (9, 1, 1) and pw.x_labels == tuple(xl) + ("ξ",) and pw.y_labels == ("q",) and pw.u_labels == ("q_err",)
    got = pw.model() + pw.model_cd()
    host = [pid_prototype.q2e_plant(Ar[k], Br[k], K[k], Kf[k], iq=xl.index("q"), i_ele=ul.index("elevator_cmd")) for k in range(28)]
    f64 = (np.array([p[0] for p in host]), np.array([p[1] for p in host])[:, :, None], np.array([p[2] for p in host])[:, None, :],
           np.array([p[3] for p in host]).reshape(28, 1, 1))
    eye, zero = np.broadcast_to(np.eye(8), (28, 8, 8)), np.zeros((28, 8, 2))
    integ = tuple(np.repeat(m[None], 28, axis=0) for m in proto.integrator())
    args = ((Ar, Br, eye, zero), integ, list(range(9)), F, G, [xl.index("q")])
    pro = proto.connect_batch(*args)
    assert all(np.array_equal(a, b) for a, b in zip(pro[:4], f64))          # (the host test's statement, on these inputs)
    long = proto.connect_batch(*args, dtype=np.longdouble)
    # D' = 0 and B' has one non-zero entry: blocks whose largest entry is 0 are held to equality
    assert np.array_equal(got[3], f64[3])
    _hold("q2e plants by connect, 28 nodes", got[:3], long[:3], f64[:3], capsys)
    P = pid_prototype.q2e_stored()
    res = fb.pid_metrics(pw, P[:, None, :], u="q_err", y="q", settings=fb.Settings(t_sim=pid_prototype.Q2E_T_SIM, dt=1e-3, w=pid_prototype.Q2E_GRID),
                         weights=pid_prototype.Q2E_WEIGHTS)
    pw.close()
    m = res.metrics[:, 0]
    with capsys.disabled():
        print(f"\n[q2e by connect, stored gains] worst over 28 nodes: Ms {m[:, 0].max():.4f}  ie {m[:, 1].max():.4f}  ef {m[:, 2].max():.4f}", end="")
    assert (res.status == 0).all()
    assert fb.check_results(m, fb.Metrics(*pid_prototype.Q2E_THRESHOLDS)).all()
    assert (m[:, 0] < 1.6).all() and (m[:, 1] < 0.3).all() and (m[:, 2] < 0.04).all()
    assert ("%.4f" % m[:, 0].max(), "%.4f" % m[:, 1].max(), "%.4f" % m[:, 2].max()) == ("1.3641", "0.0431", "0.0132")


def test_the_pitch_rate_loop_by_unity_feedback(fb, capsys):
    pw, _ = _q2e_world(fb)
    P = pid_prototype.q2e_stored()
    cw = fb.pid_world(P)
    loop = fb.unity_feedback(pw, cw, "q_err", "q")
    assert loop.ok.all() and loop.world.u_labels == ("q_ref",) and loop.world.y_labels == ("q", "u") and loop.world.nx == 11
    got = loop.world.model() + loop.world.model_cd()
    A9, B9 = pw.model()
    C9, D9 = pw.model_cd()
    host = [pid_prototype.closed_loop(A9[k], B9[k, :, 0], C9[k, 0], D9[k, 0, 0], P[k]) for k in range(28)]
    want = (np.array([h[0] for h in host]), np.array([h[1] for h in host])[:, :, None],
            np.array([[h[2][0], h[3][0]] for h in host]), np.array([[h[2][1], h[3][1]] for h in host])[:, :, None])
    plant = (A9, B9, C9, D9)
    comp = tuple(np.array([proto.pid(P[k])[j] for k in range(28)]) for j in range(4))
    F = np.zeros((2, 2)); F[0, 1] = 1.0; F[1, 0] = -1.0
    args = (plant, comp, [0, 1], F, np.array([[0.0], [1.0]]), None)
    pro, long = proto.connect_batch(*args), proto.connect_batch(*args, dtype=np.longdouble)
    # the host route's matrices sit where the prototype's do (tests/test_connect_host.py: within 4 ulp of the largest entry)
    eps = np.finfo(np.float64).eps
    for a, b in zip(pro[:4], want):
        assert float(proto.block_dev(a, b).max()) <= 4 * eps
    _hold("pitch-rate loop by unity_feedback, 28 nodes", got, long[:4], pro[:4], capsys)
    lam = fb.poles(loop.world)
    si = fb.stepinfo(loop.world, [("q_ref", "q")], pid_prototype.Q2E_T_SIM, dt=2e-3)
    with capsys.disabled():
        print(f"\n[q <- q_ref by connect] rise {si.risetime.min():.2f}-{si.risetime.max():.2f} s, settling {si.settlingtime.min():.2f}-"
              f"{si.settlingtime.max():.2f} s, overshoot {si.overshoot.min():.1f}-{si.overshoot.max():.1f} %; max Re pole {lam.poles.real.max():.2e}", end="")
    assert (lam.status == 0).all() and lam.stable.all() and si.ok.all()
    for v, lo, hi, digits in ((si.risetime, 0.13, 0.38, 2), (si.settlingtime, 0.86, 2.39, 2), (si.overshoot, 4.5, 18.6, 1)):
        assert round(float(v.min()), digits) >= lo and round(float(v.max()), digits) <= hi, (v.min(), v.max(), lo, hi)
    for w in (loop.world, cw, pw):
        w.close()
