"""fb_lss_transform and fb_lss_steady (flightbatch.surgery): the design-model surgery between linearize and lqr on the device, pinned by

  1. the longdouble restatement (tests/surgery_prototype.py): seven transform shapes (selection lists that reorder and drop, an xdot_zero
     mask) and eight steady-map shapes (K per system and K for the batch) x N in {1, 63, 130}: every P of both kernels at its smallest and
     its largest size, ny > P;
  2. rows = NULL: the host subsystem / delete_vars of the source, bit for bit;
  3. position independence and reproducibility, bit for bit, the source left as it was, the new handle a full citizen under both exchanges;
  4. the poles of T A inv(T) against the poles of A, and the DC gain from r to z under u = K_fwd r - K x against the identity;
  5. a singular and a non-finite system flagged in place among healthy ones; rpiv = 1 for T = I;
  6. the refusals of the C ABI on a live device;
  7. trim -> linearize -> linear_world -> c172x_design_model -> lqr_tracker at the 28 design nodes against the reference's stored tables.

The bound of 1, 4 and 7 is the family's rule (tests/test_gpu_connect.py): the device differs from the float64 restatement in FMA contraction
and in <= 1-ulp division only, so its deviation from the longdouble side may be ten times the prototype's over the same systems, with 1e-13
as the floor. A deviation is max|got - want| over a block divided by the block's largest |want|, per system, the worst over the batch; a
block that is zero on the longdouble side is held to equality. The measured figures are in docs/design/linearize.md, "Design-model surgery
on the device"."""
import ctypes as C
import functools

import numpy as np
import pytest

import poles_prototype
import reference_fixtures as rf
import surgery_prototype as proto
from support import LSS_EXCHANGES, clock, exchange

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-13, 10.0
T_BLOCKS = ("A'", "B'", "C'", "D'", "xdot0'", "x0'")
S_BLOCKS = ("X", "U", "K_fwd")
T_MID, S_MID = (16, 4, 33, 16, 4, 33), (14, 2)
LON = (20, 4, 38, 9, 2, 16)
ids = lambda s: "/".join(map(str, s))
pi32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
same = lambda a, b: np.array_equal(a, b, equal_nan=True)


def _lss(fb, M, keep=slice(None)):
    """the blocks (xdot0, x0, u0, y0, A, B, C, D) [n, ...] as a LinearizedSS with labels x0.., u0.., y0.."""
    xdot0, x0, u0, y0, A, B, Cm, D = (np.ascontiguousarray(b[keep]) for b in M)
    return fb.LinearizedSS(xdot0=xdot0, x0=x0, u0=u0, y0=y0, A=A, B=B, C=Cm, D=D, x_labels=tuple(f"x{k}" for k in range(A.shape[1])),
                           u_labels=tuple(f"u{k}" for k in range(B.shape[2])), y_labels=tuple(f"y{k}" for k in range(Cm.shape[1])))


def _plain(fb, S, keep=slice(None)):
    """(A, B, C, D) [n, ...] as a LinearizedSS at rest"""
    A, B, Cm, D = S
    n, nx, nu, ny = A.shape[0], A.shape[1], B.shape[2], Cm.shape[1]
    z = np.zeros
    return _lss(fb, (z((n, nx)), z((n, nx)), z((n, nu)), z((n, ny)), A, B, Cm, D), keep)


def _blocks(w):
    """(A, B, C, D, xdot0, x0, u0, y0) of a world that still sits at its linearisation point (x = x0, u = u0: f_ode returns xdot0 and y0 as they
    are, every product being a finite number times zero)"""
    A, B = w.model()
    Cm, D = w.model_cd()
    x0, u0 = w.x.T.copy(), w.u.T.copy()
    xd = np.empty((w.nx, w.n))
    w.f_ode(xd)
    return A, B, Cm, D, xd.T.copy(), x0, u0, w.y.T.copy()


def _transform(fb, cs, keep=slice(None), select=True):
    """(A', B', C', D', xdot0', x0', u0, y0, status, rpiv) of the systems `keep` of a transform case, through its selection lists"""
    M, rows, zero, ix, iu, iy = cs
    w = fb.LinearWorld(_lss(fb, M, keep))
    res = fb.transform(w, rows, xdot_zero=np.flatnonzero(zero), x=ix if select else None, u=iu if select else None, y=iy if select else None)
    assert res.world.n == w.n and (res.world.nx, res.world.nu, res.world.ny) == ((len(ix), len(iu), len(iy)) if select else (w.nx, w.nu, w.ny))
    assert res.world.x_labels == tuple(f"y{rows[k]}" for k in (ix if select else range(w.nx)))
    out = _blocks(res.world) + (res.status.copy(), res.rpiv.copy())
    res.world.close()
    w.close()
    return out


def _steady(fb, cs, keep=slice(None), wide=False):
    S, iz, K, K_wide = cs
    w = fb.LinearWorld(_plain(fb, S, keep))
    res = fb.steady_state(w, iz, K_wide if wide else K[keep])
    w.close()
    return res.X, res.U, res.K_fwd, res.status, res.rpiv


def _dev(got, want):
    """the worst over the batch of max|got - want| / max|want| per system; a system whose block is zero is held to equality"""
    got, want = np.asarray(got), np.asarray(want)
    n = want.shape[0]
    d = np.abs(got.astype(np.longdouble) - want).reshape(n, -1).max(axis=1).astype(np.float64)
    s = np.abs(want).reshape(n, -1).max(axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        return float(np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0)).max())


def _hold(label, names, got, long, f64, capsys):
    dev = [_dev(g, l) for g, l in zip(got, long)]
    pro = [_dev(f, l) for f, l in zip(f64, long)]
    with capsys.disabled():
        print(f"\n[{label}] device (prototype) vs longdouble: " + "  ".join(f"{b} {d:.2e} ({p:.2e})" for b, d, p in zip(names, dev, pro)), end="")
    for b, d, p in zip(names, dev, pro):
        assert d <= max(MARGIN * p, FLOOR), (label, b, d, p)


# ---- 1. accuracy -----------------------------------------------------------------------------------------------------------------------------------
def test_the_shapes_cover_every_group_size():
    t_sizes, s_sizes = [s[0] for s in proto.T_SHAPES], [s[0] + s[1] for s in proto.S_SHAPES]
    for P in (8, 16, 32):
        # k_transform: each P at the smallest and at the largest size that selects it; k_steady: at the largest and at a smaller one
        assert {P // 2 + 1 if P > 8 else 1, P} <= {m for m in t_sizes if proto.group(m) == P}, (P, t_sizes)
        mine = {m for m in s_sizes if proto.group(m) == P}
        assert P in mine and min(mine) < P, (P, s_sizes)
    assert any(s[2] > proto.group(s[0]) for s in proto.T_SHAPES) and LON in proto.T_SHAPES


@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("shape", proto.T_SHAPES, ids=ids)
def test_transform_against_the_longdouble_side(fb, shape, n, capsys):
    cs, f64, long = proto.t_sides(shape)
    M, rows, zero, ix, iu, iy = cs
    got = _transform(fb, cs, slice(0, n))
    assert (got[8] == 0).all() and (f64[6] == 0).all()
    sub = lambda side: proto.subsystem(tuple(b[:n] for b in side[:6]), ix, iu, iy)
    _hold(f"fb_lss_transform {ids(shape)} N {n}", T_BLOCKS, got[:6], sub(long), sub(f64), capsys)
    # what is copied or set is exact: D', x0' = y0[rows], u0, y0, and the masked entries of xdot0'
    assert same(got[3], M[7][:n][:, iy][:, :, iu]) and same(got[5], M[3][:n][:, rows][:, ix]) and same(got[6], M[2][:n][:, iu]) and same(got[7], M[3][:n][:, iy])
    assert (got[4][:, zero[ix].astype(bool)] == 0.0).all() and (got[4][:, ~zero[ix].astype(bool)] != 0.0).all()
    assert np.abs(got[9] / f64[7][:n] - 1.0).max() <= 1e-12 and ((got[9] > 0) & (got[9] <= 1)).all()


@pytest.mark.parametrize("wide", [False, True], ids=["K per system", "K batch-wide"])
@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("shape", proto.S_SHAPES, ids=ids)
def test_steady_against_the_longdouble_side(fb, shape, n, wide, capsys):
    cs, f64, long = proto.s_sides(shape, wide)
    got = _steady(fb, cs, slice(0, n), wide)
    assert (got[3] == 0).all() and (f64[3] == 0).all()
    _hold(f"fb_lss_steady {ids(shape)} N {n} {'K batch-wide' if wide else 'K per system'}", S_BLOCKS, got[:3], [b[:n] for b in long[:3]],
          [b[:n] for b in f64[:3]], capsys)
    assert np.abs(got[4] / f64[4][:n] - 1.0).max() <= 1e-12


# ---- 2. rows = NULL: subsystem and delete_vars, device to device -----------------------------------------------------------------------------------
def test_subsystem_and_delete_vars_are_the_hosts_bit_for_bit(fb):
    M, rows, zero, ix, iu, iy = proto.t_sides(LON)[0]
    lss = _lss(fb, M)
    w = fb.LinearWorld(lss)
    names = lambda labels, idx: [labels[k] for k in idx]
    xl, ul, yl = names(lss.x_labels, ix), names(lss.u_labels, iu), names(lss.y_labels, iy)
    cases = [(fb.subsystem_world(w, x=xl, u=ul, y=yl), fb.subsystem(lss, x=xl, u=ul, y=yl)),
             (fb.subsystem_world(w, x=ix, u=None, y=iy), fb.subsystem(lss, x=xl, y=yl)),
             (fb.subsystem_world(w), lss),
             (fb.delete_vars_world(w, ["x3", "u1", "y0", "y37", "nope"]), fb.delete_vars(lss, ["x3", "u1", "y0", "y37", "nope"])),
             (fb.delete_vars_world(w, "x19"), fb.delete_vars(lss, "x19"))]
    for got, want in cases:
        assert (got.x_labels, got.u_labels, got.y_labels) == (tuple(want.x_labels), tuple(want.u_labels), tuple(want.y_labels))
        b = _blocks(got)
        for g, h in zip(b, (want.A, want.B, want.C, want.D, want.xdot0, want.x0, want.u0, want.y0)):
            assert g.shape == np.asarray(h).shape and same(g, h)
        got.close()
    # the lists, the status and rpiv of the C ABI with rows = NULL; an xdot_zero mask still sets its entries
    st, rp = np.full(w.n, -1, dtype=np.int32), np.zeros(w.n)
    h = C.c_void_p()
    mask = np.zeros(w.nx, dtype=np.int32); mask[ix[0]] = 1
    assert fb.lib.fb_lss_transform(w._h, None, pi32(mask), pi32(ix), len(ix), None, 0, None, 0, pi32(st), pd(rp), C.byref(h)) == 0, fb.lib.fb_last_error()
    got = fb.LinearWorld(_handle=h, _labels=(tuple(xl), lss.u_labels, lss.y_labels))
    b = _blocks(got)
    assert (st == 0).all() and (rp == 1.0).all() and (got.nx, got.nu, got.ny) == (len(ix), w.nu, w.ny)
    assert (b[4][:, 0] == 0.0).all() and same(b[4][:, 1:], M[0][:, ix[1:]]) and same(b[0], M[4][:, ix][:, :, ix])
    got.close()
    w.close()


# ---- 3. bit for bit --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _t_mid(fb):
    out = _transform(fb, proto.t_sides(T_MID)[0])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _s_mid(fb):
    out = _steady(fb, proto.s_sides(S_MID)[0])
    for a in out:
        a.setflags(write=False)
    return out


def test_a_second_call_and_the_batch_in_another_order(fb):
    for full, run, cs in ((_t_mid(fb), _transform, proto.t_sides(T_MID)[0]), (_s_mid(fb), _steady, proto.s_sides(S_MID)[0])):
        assert all(same(a, b) for a, b in zip(full, run(fb, cs)))
        assert all(same(a, b[::-1]) for a, b in zip(full, run(fb, cs, slice(None, None, -1))))
        keep = np.array([129, 3, 64, 63, 0, 77, 12])
        assert all(same(a[keep], b) for a, b in zip(full, run(fb, cs, keep)))
        for i in (0, 63, 129):      # system i alone
            assert all(same(a[i:i + 1], b) for a, b in zip(full, run(fb, cs, slice(i, i + 1))))
        assert all(same(a[:63], b) for a, b in zip(full, run(fb, cs, slice(0, 63))))


def test_batch_wide_k_is_the_replicated_one(fb):
    S, iz, K, K_wide = proto.s_sides(S_MID)[0]
    n = 63
    rep = (tuple(b[:n] for b in S), iz, np.repeat(K_wide[None], n, axis=0), K_wide)
    per, wide = _steady(fb, rep), _steady(fb, rep, wide=True)
    assert (per[3] == 0).all() and all(same(a, b) for a, b in zip(per, wide))
    # without K: the same X and U, no K_fwd
    w = fb.LinearWorld(_plain(fb, rep[0]))
    res = fb.steady_state(w, iz)
    w.close()
    assert res.K_fwd is None and same(res.X, per[0]) and same(res.U, per[1])


def test_the_source_is_left_as_it_was(fb):
    cs = proto.t_sides(T_MID)[0]
    M, rows, zero, ix, iu, iy = cs
    w = fb.LinearWorld(_lss(fb, M))
    rng = np.random.default_rng(8)
    w.set_params(dt=0.004)
    w.u = rng.standard_normal((w.nu, w.n))
    w.log_configure(every=2, capacity=8, y=[0, 1], x=[0])
    w.step(7)
    w.sync()

    def snapshot():
        t, data = w.log_read()
        return (w.x, w.u, w.status, np.array(clock(fb, w)), t, data) + w.model() + w.model_cd()
    before = snapshot()
    res = fb.transform(w, rows, xdot_zero=np.flatnonzero(zero), x=ix, u=iu, y=iy)
    st = fb.steady_state(w, list(range(w.nu)))
    after = snapshot()
    assert all(same(a, b) for a, b in zip(before, after)) and st.status.shape == (w.n,)
    assert clock(fb, w) == (pytest.approx(7 * 0.004), 7)
    # the new handle: the source's dt, at its own linearisation point, clock at zero
    a = res.world
    assert clock(fb, a) == (0.0, 0) and (a.status == 0).all()
    assert all(same(p, q) for p, q in zip(_blocks(a), _t_mid(fb)[:8]))
    a.step(1)
    a.sync()
    assert clock(fb, a) == (pytest.approx(0.004), 1)
    a.close()
    w.close()


@pytest.mark.parametrize("xch", LSS_EXCHANGES)
def test_the_new_handle_is_an_ordinary_one(fb, xch):
    cs = proto.t_sides((8, 2, 9, 8, 2, 9))[0]
    M, rows, zero, ix, iu, iy = cs
    with exchange(xch):
        w = fb.LinearWorld(_lss(fb, M))
        res = fb.transform(w, rows, xdot_zero=np.flatnonzero(zero), x=ix, u=iu, y=iy)
        a = res.world
        A, B, Cm, D, xd0, x0, u0, y0 = _blocks(a)
        n = a.n
        b = fb.LinearWorld(fb.LinearizedSS(xdot0=xd0, x0=x0, u0=u0, y0=y0, A=A, B=B, C=Cm, D=D, x_labels=a.x_labels, u_labels=a.u_labels,
                                           y_labels=a.y_labels))
        assert a.exchange == b.exchange == xch and all(same(p, q) for p, q in zip(_blocks(a), _blocks(b)))
        assert a.u_labels == tuple(f"u{k}" for k in iu) and a.y_labels == tuple(f"y{k}" for k in iy)
        rng = np.random.default_rng(11)
        xs, u = rng.standard_normal((a.nx, n)), rng.standard_normal((a.nu, n))
        outs = []
        for v in (a, b):
            v.set_state(xs)
            v.set_params(dt=0.003)
            v.u = u
            xd = np.empty((v.nx, n))
            v.f_ode(xd)
            y1 = v.y
            assert fb.lib.fb_set_steps_per_launch(v._h, 7) == 0
            v.step(50)
            v.sync()
            v.f_ode()
            outs.append((xd, y1, v.x, v.y, np.array(clock(fb, v))))
        assert all(same(p, q) for p, q in zip(*outs)) and np.isfinite(outs[0][2]).all() and outs[0][2].any()
        # and the design verbs take it
        assert same(fb.poles(a).poles, fb.poles(b).poles)
        for v in (a, b, w):
            v.close()


# ---- 4. independent properties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [8, 17])
def test_a_similarity_keeps_the_poles(fb, nx, capsys):
    """poles(T A inv(T)) against poles(A), both on the device, by tests/test_gpu_poles.py's bound (ten times the prototype's figure, 1e-11 as
    the floor); the prototype's figure here is LAPACK on the float64 restatement's T A inv(T) against LAPACK on A"""
    n = 130
    rng = np.random.default_rng([proto.SEED, 4, nx])
    A = poles_prototype.systems(nx, n)
    T = proto.well_conditioned(rng, n, nx)
    z = np.zeros
    M = (z((n, nx)), z((n, nx)), z((n, 1)), z((n, nx)), A, np.ones((n, nx, 1)), T, z((n, nx, 1)))
    w = fb.LinearWorld(_lss(fb, M))
    res = fb.transform(w, list(range(nx)))
    src, new = fb.poles(w), fb.poles(res.world)
    res.world.close()
    w.close()
    assert (res.status == 0).all() and (src.status == 0).all() and (new.status == 0).all()
    mu = np.array([np.linalg.eigvals(a) for a in A])
    Ap = proto.transform_batch(M, list(range(nx)))[0]
    d = poles_prototype.batch_dev(new.poles, src.poles)
    p = poles_prototype.batch_dev(np.array([np.linalg.eigvals(a) for a in Ap]), mu)
    with capsys.disabled():
        print(f"\n[poles of T A inv(T) vs poles of A] nx {nx} x {n}: {d:.2e} (LAPACK on the prototype's {p:.2e})", end="")
    assert d <= max(MARGIN * p, 1e-11)


@pytest.mark.parametrize("shape", [(6, 2), (16, 8), (17, 1)], ids=ids)
def test_the_dc_gain_from_r_to_z_is_the_identity(fb, shape, capsys):
    cs, f64, _ = proto.s_sides(shape)
    S, iz, K, _ = cs
    got = _steady(fb, cs)
    n, nz = proto.N_SYS, shape[1]
    eye = np.broadcast_to(np.eye(nz, dtype=np.longdouble), (n, nz, nz))
    gain = lambda Kf: np.array([proto.dc_gain(tuple(b[i] for b in S), iz, K[i], Kf[i]) for i in range(n)])
    _hold(f"DC gain r -> z under u = K_fwd r - K x, {ids(shape)}", ("gain",), [gain(got[2])], [eye], [gain(f64[2])], capsys)


# ---- 5. failures in place --------------------------------------------------------------------------------------------------------------------------
def test_flagged_systems_among_healthy_ones(fb):
    n, sing, nanf = 65, 17, 40
    # transform. The family's rule flags a pivot that IS zero: a T that is singular only to rounding shows in rpiv, not in the status word. So
    # T is exact here, every system its own row permutation of a diagonal of powers of two (each elimination step is exact, as for the
    # unit rows of the reference's T); one system's C has row rows[2] again in row rows[5]'s place (`rows` is the batch's: the repeated row
    # is in the data), one has a NaN in B
    M, rows, zero, ix, iu, iy = proto.t_sides((8, 2, 9, 8, 2, 9))[0]
    M = [b[:n].copy() for b in M]
    rng = np.random.default_rng(21)
    for i in range(n):
        M[6][i][rows] = np.diag(2.0 ** rng.integers(-3, 4, 8))[rng.permutation(8)]
    M[6][sing][rows[5]] = M[6][sing][rows[2]]
    M[5][nanf, 3, 1] = np.nan
    cs = (M, rows, zero, ix, iu, iy)
    got = _transform(fb, cs)
    expect = np.zeros(n, dtype=np.int32); expect[sing] = fb.K["FB_SURGERY_SINGULAR"]; expect[nanf] = fb.K["FB_SURGERY_NOT_FINITE"]
    assert np.array_equal(got[8], expect), got[8]
    for b in got[:4]:
        assert np.isnan(b[sing]).all() and np.isnan(b[nanf]).all()
    assert got[9][sing] == 0.0 and np.isnan(got[9][nanf])
    healthy = np.flatnonzero(expect == 0)
    ref = _transform(fb, cs, healthy)
    assert healthy.size == 63 and (ref[8] == 0).all() and all(same(a[healthy], b) and np.isfinite(b).all() for a, b in zip(got, ref))
    assert np.array_equal(proto.transform_batch(M, rows, zero)[6], expect)
    # a repeated entry of `rows` itself: every system is singular
    twice = rows.copy(); twice[5] = twice[2]
    w = fb.LinearWorld(_lss(fb, M, healthy))
    res = fb.transform(w, twice)
    assert (res.status == fb.K["FB_SURGERY_SINGULAR"]).all() and (res.rpiv == 0.0).all() and np.isnan(res.world.model()[0]).all()
    res.world.close()
    # T = I: every pivot is 1
    eye = [b.copy() for b in M]
    eye[6][:, rows] = np.eye(8)
    eye[5][nanf, 3, 1] = 0.5
    w2 = fb.LinearWorld(_lss(fb, eye))
    res = fb.transform(w2, rows)
    assert (res.status == 0).all() and (res.rpiv == 1.0).all()
    res.world.close()
    w.close(); w2.close()
    # the steady map: an all-zero column of L, a NaN in K
    S, iz, K, K_wide = proto.s_sides((6, 2))[0]
    S, K = [b[:n].copy() for b in S], K[:n].copy()
    S[0][sing][:, 3] = 0.0; S[2][sing][:, 3] = 0.0
    K[nanf, 1, 4] = np.nan
    cs = (S, iz, K, K_wide)
    got = _steady(fb, cs)
    assert np.array_equal(got[3], expect), got[3]
    for b in got[:3]:
        assert np.isnan(b[sing]).all() and np.isnan(b[nanf]).all()
    assert got[4][sing] == 0.0 and np.isnan(got[4][nanf])
    ref = _steady(fb, cs, healthy)
    assert (ref[3] == 0).all() and all(same(a[healthy], b) and np.isfinite(b).all() for a, b in zip(got, ref))
    assert np.array_equal(proto.steady_batch(S, iz, K)[3], expect)


# ---- 6. refusals on a live device ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 5
    rng = np.random.default_rng(3)
    mk = lambda nx, nu, ny: fb.LinearWorld(_plain(fb, tuple(rng.standard_normal(s) for s in ((n, nx, nx), (n, nx, nu), (n, ny, nx), (n, ny, nu)))))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    arr = lambda v: None if v is None else np.array(v, dtype=np.int32)

    def transform(h, rows=(0, 1, 2), ix=None, iu=None, iy=None, counts=None, out=True, timed=True):
        if timed:
            assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        r, jx, ju, jy = arr(rows), arr(ix), arr(iu), arr(iy)
        cnt = counts or tuple(0 if j is None else len(j) for j in (jx, ju, jy))
        new = C.c_void_p(1)
        rc = fb.lib.fb_lss_transform(h, pi32(r), None, pi32(jx), cnt[0], pi32(ju), cnt[1], pi32(jy), cnt[2], None, None, C.byref(new) if out else None)
        err = fb.lib.fb_last_error()
        if rc == 0:
            fb.lib.fb_destroy(new)
        else:
            assert not out or not new.value       # no handle behind a refusal
        return rc, err, (launches(h) if timed else 0)

    def steady(h, iz=(0, 1), nz=None, K=False, Kfwd=False, timed=True):
        if timed:
            assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        j = arr(iz)
        buf = np.zeros(32 * 32 * n)
        rc = fb.lib.fb_lss_steady(h, pi32(j), (len(iz) if iz is not None else 0) if nz is None else nz, pd(buf) if K else None, 0, None, None,
                                  pd(buf) if Kfwd else None, None, None)
        return rc, fb.lib.fb_last_error(), (launches(h) if timed else 0)

    def refused(call, verb, h, cause, **kw):
        rc, err, nl = call(h, **kw)
        assert rc != 0 and verb in err and cause in err and nl == 0, (cause, err, nl)

    t, s = (transform, b"fb_lss_transform"), (steady, b"fb_lss_steady")
    r = fb.Robot2DWorld(n)
    for call in (t, s):
        rc, err, _ = call[0](None, timed=False)
        assert rc != 0 and b"null handle" in err
        refused(*call, r._h, b"not a LinearizedSS handle", timed=False)      # (a Robot2D handle keeps no per-launch stamps)
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.transform(r, [0])
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.steady_state(r, [0])
    r.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 2, 4, n, 0, C.byref(h)) == 0
    for call in (t, s):
        refused(*call, h, b"no model yet")
    fb.lib.fb_destroy(h)
    w = mk(3, 2, 4)
    refused(*t, w._h, b"out is null", out=False)
    refused(*t, w._h, b"rows[2] = 4 is outside [0, 4)", rows=(0, 1, 4))
    refused(*t, w._h, b"rows[0] = -1 is outside", rows=(-1, 1, 2))
    refused(*t, w._h, b"ix[1] = 3 is outside [0, 3)", ix=(0, 3))
    refused(*t, w._h, b"iu[0] = 2 is outside [0, 2)", iu=(2,))
    refused(*t, w._h, b"iy[0] = 4 is outside [0, 4)", iy=(4,))
    refused(*t, w._h, b"nxo = 0", ix=(0,), counts=(0, 0, 0))
    refused(*t, w._h, b"nxo = 4", ix=(0, 1, 2, 0))
    refused(*t, w._h, b"nuo = 3", iu=(0, 1, 0))
    refused(*t, w._h, b"nyo = 0", iy=(0,), counts=(0, 0, 0))
    refused(*t, w._h, b"nyo = 5", iy=(0,) * 5)
    for kw in (dict(), dict(rows=None), dict(rows=None, ix=(2, 0), iu=(1,), iy=(3, 3, 0))):      # (an index may repeat in a selection)
        rc, err, nl = transform(w._h, **kw)
        assert rc == 0 and nl == 1, err
    refused(*s, w._h, b"nz = 1", iz=(0,))
    refused(*s, w._h, b"nz = 3", iz=(0, 1, 2))
    refused(*s, w._h, b"iz is required", iz=None, nz=2)
    refused(*s, w._h, b"iz[1] = 4 is outside [0, 4)", iz=(0, 4))
    refused(*s, w._h, b"needs K", Kfwd=True)
    for kw in (dict(), dict(K=True), dict(K=True, Kfwd=True)):
        rc, err, nl = steady(w._h, **kw)
        assert rc == 0 and nl == 1, err
    big = mk(25, 8, 8)
    refused(*s, big._h, b"nx + nu = 33", iz=tuple(range(8)))
    full = mk(32, 1, 1)
    refused(*s, full._h, b"nx = 32", iz=(0,))
    with pytest.raises(KeyError, match="not an output label"):
        fb.transform(w, ["y0", "y1", "nope"])
    with pytest.raises(ValueError, match="new states for a world of 3"):
        fb.transform(w, [0, 1])
    with pytest.raises(ValueError, match="xdot_zero"):
        fb.transform(w, [0, 1, 2], xdot_zero=[3])
    for x in (w, big, full):
        x.close()


# ---- 7. end to end against what the reference stores -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _design_worlds(fb):
    """trim -> linearize -> linear_world -> c172x_design_model at the 28 design nodes: (host LinearizedSS, source world, full, lon, lat results)"""
    EAS, h, flaps = rf.design_nodes()
    w = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme="onesided2")
    src = fb.linear_world(w)
    w.close()
    assert lss.success.all() and (lss.status == 0).all()
    return lss, src, fb.c172x_design_model(src), fb.c172x_design_model(src, "lon"), fb.c172x_design_model(src, "lat")


def test_the_design_model_of_the_28_nodes(fb, capsys):
    import reference_lqr as rl
    lss, src, full, lon, lat = _design_worlds(fb)
    assert full.ok.all() and lon.ok.all() and lat.ok.all()
    assert full.world.x_labels == tuple(rl.XP_LABELS) and full.world.y_labels == tuple(lss.y_labels) and (full.world.nx, full.world.nu, full.world.ny) == (20, 4, 38)
    assert lon.world.x_labels[:9] == ("q", "θ", "EAS", "α", "h", "α_filt", "n_eng", "thr_p", "ele_p") and (lon.world.nx, lon.world.nu, lon.world.ny) == (9, 2, 16)
    assert lat.world.x_labels == ("p", "r", "ψ", "φ", "EAS", "β", "β_filt", "ail_p", "rud_p") and (lat.world.nx, lat.world.nu, lat.world.ny) == (9, 2, 13)
    # the source world is the host's LinearizedSS, and the prototype on it gives the device's design model by the accuracy rule
    M = (lss.xdot0, lss.x0, lss.u0, lss.y0, lss.A, lss.B, lss.C, lss.D)
    assert all(same(g, h) for g, h in zip(_blocks(src), (lss.A, lss.B, lss.C, lss.D, lss.xdot0, lss.x0, lss.u0, lss.y0)))
    rows = [lss.y_labels.index(s) for s in rl.XP_LABELS]
    zero = np.array([s in ("EAS", "α", "β", "n_eng") for s in rl.XP_LABELS])
    f64, long = proto.transform_batch(M, rows, zero), proto.transform_batch(M, rows, zero, np.longdouble)
    got = _blocks(full.world)
    assert (f64[6] == 0).all() and np.abs(full.rpiv / f64[7] - 1.0).max() <= 1e-12
    _hold("c172x_design_model, 28 nodes, full", T_BLOCKS, got[:6], long[:6], f64[:6], capsys)
    assert (got[4][:, zero] == 0.0).all() and same(got[5], lss.y0[:, rows]) and same(got[6], lss.u0) and same(got[7], lss.y0)
    # lon and lat are subsystems of it, bit for bit; the distance to the tree's host route (reference_lqr.design_model: its T has exact unit
    # rows and 1 / ω_rated where the device's has the Jacobian's rows) is printed, the gain tables below are the check of the chain
    for res in (lon, lat):
        v = res.world
        ix, iu, iy = ([labels.index(s) for s in sel] for labels, sel in ((rl.XP_LABELS, v.x_labels), (lss.u_labels, v.u_labels), (lss.y_labels, v.y_labels)))
        assert all(same(g, h) for g, h in zip(_blocks(v)[:6], proto.subsystem(got[:6], ix, iu, iy))) and same(res.rpiv, full.rpiv)
    iy = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    host = [rl.design_model(lss.A[k], lss.B[k], lss.C[k][iy]) for k in range(28)]
    d = max(_dev(got[0], np.array([p[0] for p in host])), _dev(got[1], np.array([p[1] for p in host])))
    with capsys.disabled():
        print(f"\n[c172x_design_model vs the host route of tests/reference_lqr.py] A', B': {d:.2e}; rpiv {full.rpiv.min():.2e} - {full.rpiv.max():.2e}", end="")


def test_the_references_gain_tables_with_no_model_coming_home(fb, capsys):
    import reference_lqr as rl
    lss, src, full, lon, lat = _design_worlds(fb)
    lon_red, lat_red = fb.delete_vars_world(lon.world, "h"), fb.delete_vars_world(lat.world, "ψ")
    assert lon_red.x_labels == tuple(rl.LON_RED) and lat_red.x_labels == tuple(rl.LAT_RED)
    for name, (xl, ul, zl, qx, qi, r, fwd) in rl.DESIGNS.items():
        world = {tuple(rl.LON_RED): lon_red, tuple(rl.LON_FULL): lon.world, tuple(rl.LAT_RED): lat_red}[tuple(xl)]
        assert world.x_labels == tuple(xl) and world.u_labels == tuple(ul)
        q = np.array([float(qx.get(k, 0.0)) for k in xl])
        K_fbk, K_fwd, K_int, status = fb.lqr_tracker(world, zl, q, np.array(r, dtype=np.float64), None if qi is None else np.array(qi, dtype=np.float64),
                                                     forward=fwd)
        assert (status == 0).all(), (name, status)
        st = rf.stored(name)
        got = {"K_fbk": K_fbk, "K_fwd": K_fwd, "K_int": K_int}
        dev = {}
        for m in got:
            want = np.moveaxis(st[m], -1, 0)
            assert got[m].shape == want.shape, (name, m, got[m].shape, want.shape)
            scale = np.abs(want).reshape(28, -1).max(axis=1)
            dev[m] = float((np.abs(got[m] - want).reshape(28, -1).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())
        line = f"\n[lqr_tracker {name:10s}] vs the stored tables K_fbk {dev['K_fbk']:.2e}  K_fwd {dev['K_fwd']:.2e}  K_int {dev['K_int']:.2e}"
        if fwd == "identity":
            assert same(K_fwd, np.broadcast_to(np.eye(len(zl)), K_fwd.shape))
        else:
            # K_fwd of the device against the prototype on the device's own design model and K_fbk
            A, B = world.model()
            Cm, D = world.model_cd()
            iz = [world.y_labels.index(s) for s in zl]
            pro, long = proto.steady_batch((A, B, Cm, D), iz, K_fbk), proto.steady_batch((A, B, Cm, D), iz, K_fbk, np.longdouble)
            d, p = _dev(K_fwd, long[2]), _dev(pro[2], long[2])
            line += f"; K_fwd vs longdouble on the same model {d:.2e} (prototype {p:.2e})"
            assert d <= max(MARGIN * p, FLOOR), (name, d, p)
        with capsys.disabled():
            print(line, end="")
        assert max(dev.values()) <= 5e-6, (name, dev)
    lon_red.close(); lat_red.close()


def test_the_integral_augmentation_is_the_references(fb):
    """A_aug = [A 0; C_z 0], B_aug = [B; D_z] (c172x_design.jl:354-355) from connect, exactly: with |D_z| < 1 the unit rows are the pivots of
    I - F D[jz, :], and every product is by 0 or by 1"""
    S, iz, _, _ = proto.s_sides((6, 2))[0]
    S = S[:3] + (np.clip(S[3], -0.9, 0.9),)
    w = fb.LinearWorld(_plain(fb, S))
    aug = fb.integral_augmentation(w, iz)
    A, B = aug.model()
    assert (aug.nx, aug.nu, aug.ny) == (8, 2, w.ny) and aug.x_labels == w.x_labels + tuple(f"ξ_y{k}" for k in iz) and aug.u_labels == w.u_labels
    want_A = np.concatenate([np.concatenate([S[0], np.zeros((w.n, 6, 2))], axis=2), np.concatenate([S[2][:, iz], np.zeros((w.n, 2, 2))], axis=2)], axis=1)
    assert same(A, want_A) and same(B, np.concatenate([S[1], S[3][:, iz]], axis=1))
    aug.close()
    w.close()
