"""fb_lss_c2d and the sampled models it makes (flightbatch.c2d, LinearWorld.step on a sampled world, timeresp.step / stepinfo on it and with
method="zoh", timeresp.lsim), pinned by

  1. the exact side (scipy.linalg.expm of [[A, B, xdot0], [0]] Ts) on random stable plants on both sides of every group-size edge, through the
     numpy restatement of the kernel (tests/c2d_prototype.py; tests/test_c2d_host.py holds the prototype itself to the exact side first and
     checks that the cases are fair); what is copied is copied bit for bit;
  2. neighbouring groups of a wave that square a different number of times;
  3. batch shapes, a second call, the reversed batch, bit for bit; the source left as it was;
  4. a singular and an unstable A;
  5. failure systems flagged in place among healthy neighbours;
  6. the sampled stepper: both exchanges, 1 / 7 / 50 steps per launch, the clock, a changed dt;
  7. the sampled StepInfo: samples against the exact samples, indices against the prototype's, strides, method="rk4" untouched;
  8. the two StepInfo tables the reference's robot2d design notebook stores, with method="zoh";
  9. lsim on the demo's input, and the sample at a change of input;
 10. the refusals of the C ABI on a live device.

The shared bound (the family's rule): the device differs from the prototype in FMA contraction only, so it may deviate from the exact side ten
times as far as the prototype does over the same systems, with a floor of 1e-11, every block scaled by its largest exact entry (samples: by
max|y| of the pair).

How delta is read: fb_lss_get_model returns Phi and Gamma; a sampled world fresh from c2d sits at x = x0, u = u0, so one step takes it to
x0 + delta (every product of the step is a product with an exact zero). Where delta itself is compared, the source's x0 is zero; where bits
are compared, x0 + delta is."""
import ctypes as C
import functools

import numpy as np
import pytest

import c2d_prototype as proto
import timeresp_prototype as tr
from support import clock, exchange

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = proto.FLOOR, proto.MARGIN


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _blocks(fb, M, Ts, keep=slice(None)):
    """c2d of the systems `keep` of M on the device: dict of Phi, Gamma, xp (= x0 + delta: the state after one step from the linearisation
    point), C, D, x0, u0, y0 as the sampled world holds them, squarings and status"""
    src = fb.LinearWorld(proto.model(fb, M, keep))
    res = fb.c2d(src, Ts)
    w = res.world
    assert w.Ts == Ts and src.Ts == 0.0 and w.params.dt == Ts and clock(fb, w) == (0.0, 0) and w.squarings is res.squarings
    assert (w.x_labels, w.u_labels, w.y_labels) == (src.x_labels, src.u_labels, src.y_labels)
    out = dict(status=res.status.copy(), squarings=res.squarings.copy(), x0=w.x.T.copy(), u0=w.u.T.copy())
    w.f_ode()
    out["y0"] = w.y.T.copy()
    out["Phi"], out["Gamma"] = w.model()
    out["C"], out["D"] = w.model_cd()
    w.step(1)
    w.sync()
    out["xp"] = w.x.T.copy()
    assert clock(fb, w) == (Ts, 1)
    w.close()
    src.close()
    return out


def _same_blocks(a, b, sel=slice(None)):
    return all(_same(a[k], b[k][sel]) for k in ("Phi", "Gamma", "xp", "C", "D", "x0", "u0", "y0")) and np.array_equal(a["squarings"], b["squarings"][sel]) \
        and np.array_equal(a["status"], b["status"][sel])


# ---- 1. every size against the exact side ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", proto.NU_ALL)
@pytest.mark.parametrize("nx", proto.NX_ALL)
def test_blocks_against_the_exact_side(fb, nx, nu, capsys):
    M = list(proto.plants(nx, nu))
    M[1] = np.zeros_like(M[1])          # x0 = 0: the step from the linearisation point returns delta itself
    xd0, x0, u0, y0, A, B, Cm, D = M
    for Ts in proto.TS_ALL:
        got = _blocks(fb, M, Ts)
        p = proto.c2d_batch(A, B, xd0, Ts)
        ex = proto.exact_batch(A, B, xd0, Ts)
        dev3 = (got["Phi"], got["Gamma"], got["xp"])
        d, dp, dd = proto.worst_dev(dev3, ex), proto.worst_dev(p[:3], ex), proto.worst_dev(dev3, p[:3])
        with capsys.disabled():
            print(f"\n[fb_lss_c2d vs expm] nx {nx:2d}, nu {nu}, Ts {Ts:g}, {proto.N_SYS} systems, s <= {int(got['squarings'].max())}: worst block deviation "
                  f"{d:.2e} (prototype {dp:.2e}; device vs prototype {dd:.2e})", end="")
        assert (got["status"] == 0).all() and (p[4] == 0).all() and np.array_equal(got["squarings"], p[3])
        assert d <= max(MARGIN * dp, FLOOR)
        assert _same(got["C"], Cm) and _same(got["D"], D) and _same(got["x0"], x0) and _same(got["u0"], u0) and _same(got["y0"], y0)


# ---- 2. different s inside one wave ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [7, 17])
def test_neighbouring_groups_square_a_different_number_of_times(fb, nx, capsys):
    M = proto.scaled(nx)
    got = _blocks(fb, M, 0.25)
    s = proto.c2d_batch(M[4], M[5], M[0], 0.25)[3]
    with capsys.disabled():
        print(f"\n[fb_lss_c2d, one plant times 1, 8, 64] nx {nx}: squarings {got['squarings'].tolist()}", end="")
    assert (got["status"] == 0).all() and np.array_equal(got["squarings"], s) and len(set(s.tolist())) == 3
    for i in range(proto.N_SYS):
        assert _same_blocks(_blocks(fb, M, 0.25, [i]), got, [i]), i


# ---- 3. batch shapes, repeatability, the source untouched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [8, 9, 32])
def test_batch_shapes_give_the_same_bits_and_the_source_is_untouched(fb, nx):
    M = proto.plants(nx, 2, 130)
    big = _blocks(fb, M, 0.25)
    assert (big["status"] == 0).all()
    for n in (1, 3, 9, 63):
        assert _same_blocks(_blocks(fb, M, 0.25, slice(0, n)), big, slice(0, n)), n
    assert _same_blocks(_blocks(fb, M, 0.25), big)
    assert _same_blocks(_blocks(fb, M, 0.25, slice(None, None, -1)), big, slice(None, None, -1))

    rng = np.random.default_rng(nx)
    src = fb.LinearWorld(proto.model(fb, M, slice(0, 9)))
    src.x = rng.standard_normal((nx, 9))
    src.u = rng.standard_normal((2, 9))
    src.step(7, dt=1e-3)
    src.sync()
    snap = lambda: (src.x, src.u, *clock(fb, src), src.status, *src.model(), *src.model_cd(), src.params.dt, src.Ts)
    before = snap()
    res = fb.c2d(src, 0.25)
    after = snap()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[3] == 7 and (res.status == 0).all() and res.ok.all() and res.Ts == 0.25
    Phi, Gam = res.world.model()
    assert _same(Phi, big["Phi"][:9]) and _same(Gam, big["Gamma"][:9])          # (whatever state the source is in)
    res.world.close()
    src.close()


# ---- 4. a singular and an unstable A -----------------------------------------------------------------------------------------------------------------------
def test_singular_and_unstable_plants(fb, capsys):
    one = lambda v: np.array(v, dtype=np.float64)
    for name, A, B in (("integrator chain", one([[0, 1], [0, -2]]), one([[0], [1]])), ("1 / (s - 20)", one([[20]]), one([[1]]))):
        nx = A.shape[0]
        M = (np.ones((1, nx)), np.zeros((1, nx)), np.zeros((1, 1)), np.zeros((1, 1)), A[None], B[None], np.ones((1, 1, nx)), np.zeros((1, 1, 1)))
        got = _blocks(fb, M, 0.01)
        p, ex = proto.c2d_batch(M[4], M[5], M[0], 0.01), proto.exact_batch(M[4], M[5], M[0], 0.01)
        dev3 = (got["Phi"], got["Gamma"], got["xp"])
        d, dp = proto.worst_dev(dev3, ex), proto.worst_dev(p[:3], ex)
        with capsys.disabled():
            print(f"\n[fb_lss_c2d, {name}] Ts 0.01: status {got['status'].tolist()}, s {got['squarings'].tolist()}, worst block deviation {d:.2e} "
                  f"(prototype {dp:.2e})", end="")
        assert (got["status"] == 0).all() and np.array_equal(got["squarings"], p[3])
        assert d <= max(MARGIN * dp, FLOOR)


# ---- 5. failure systems in place ---------------------------------------------------------------------------------------------------------------------------
def test_failure_systems_are_flagged_in_place(fb):
    M = [b.copy() for b in proto.plants(5, 2, 7)]
    M[4][2, 1, 3] = np.nan
    M[4][4] = 1e12 * np.eye(5)
    got = _blocks(fb, M, 1.0)
    assert got["status"].tolist() == [0, 0, proto.NOT_FINITE, 0, proto.RANGE, 0, 0]
    p = proto.c2d_batch(M[4], M[5], M[0], 1.0)
    assert np.array_equal(got["status"], p[4]) and np.array_equal(got["squarings"], p[3]) and got["squarings"][2] == got["squarings"][4] == 0
    for i in (2, 4):
        assert np.isnan(got["Phi"][i]).all() and np.isnan(got["Gamma"][i]).all() and np.isnan(got["xp"][i]).all()
        assert _same(got["C"][i], M[6][i]) and _same(got["D"][i], M[7][i])
    keep = [0, 1, 3, 5, 6]
    healthy = _blocks(fb, M, 1.0, keep)
    assert (healthy["status"] == 0).all() and _same_blocks(healthy, got, keep)
    assert not np.isnan(healthy["Phi"]).any() and not np.isnan(healthy["xp"]).any()
    src = fb.LinearWorld(proto.model(fb, [np.array([[0.0]]), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), np.array([[[2000.0]]]),
                                          np.ones((1, 1, 1)), np.ones((1, 1, 1)), np.zeros((1, 1, 1))]))
    res = fb.c2d(src, 1.0)          # e^2000 overflows
    assert res.status.tolist() == [proto.NOT_FINITE] and np.isnan(res.world.model()[0]).all()
    res.world.close()
    src.close()


# ---- 6. the sampled stepper --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", proto.STEP_NX)
def test_the_sampled_stepper(fb, nx, capsys):
    M = proto.plants(nx, 2)
    xd0, x0, u0, y0, A, B, Cm, D = M
    Ts, N, every = proto.STEP_TS, proto.STEP_N, proto.STEP_EVERY
    Phi, Gam, dl = proto.c2d_batch(A, B, xd0, Ts)[:3]
    u = u0.copy()
    u[:, 1] += 1.0
    runs = {}
    for xch in ("panel", "shfl"):
        for spl in (1, 7, 50):
            with exchange(xch):
                src = fb.LinearWorld(proto.model(fb, M))
                w = fb.c2d(src, Ts).world
            assert w.exchange == xch
            w.u = u.T
            ys = []
            for k in range(0, N + 1, every):
                w.f_ode()
                ys.append(w.y.T.copy())
                t, cnt = clock(fb, w)
                assert cnt == k and t == pytest.approx(k * Ts, rel=1e-12, abs=0.0)
                if k < N:
                    w.step(every, steps_per_launch=spl)
            w.sync()
            runs[xch, spl] = (np.array(ys), w.x.T.copy())
            if (xch, spl) == ("panel", 50):
                w.set_params(dt=2 * Ts)
                with pytest.raises(fb.FlightBatchError, match="a sampled model steps by its own sample time only"):
                    w.step(1)
                assert clock(fb, w)[1] == N
                w.set_params(dt=Ts)
                w.step(1)
                assert clock(fb, w)[1] == N + 1
                with pytest.raises(fb.FlightBatchError, match="no derivative"):
                    w.f_ode(np.empty((nx, proto.N_SYS)))
            w.close()
            src.close()
    ys, xs = runs["panel", 50]
    x, worst = x0.copy(), 0.0
    for j, k in enumerate(range(0, N + 1, every)):
        y = proto.outputs(Cm, D, x0, u0, y0, x, u)
        worst = max(worst, float((np.abs(ys[j] - y) / np.maximum(np.abs(y), 1.0)).max()))
        x = proto.map_steps(Phi, Gam, dl, x0, u0, x, u, every)
    with capsys.disabled():
        print(f"\n[fb_step on a sampled world vs the prototype's map] nx {nx:2d}, {N} steps of {Ts}: outputs {worst:.2e} of max(|y|, 1)", end="")
    assert worst <= 1e-11
    for key, (y2, x2) in runs.items():
        assert _same(y2, ys) and _same(x2, xs), key


# ---- 7. the sampled StepInfo -------------------------------------------------------------------------------------------------------------------------------
N_SI = int(round(proto.SI_TSIM / proto.SI_TS))


@functools.lru_cache(maxsize=None)
def _si_reference(nx):
    sysm, P, Pe = proto.stepinfo_case(nx)
    Y, Ye = proto.samples_map(*P, N_SI), proto.samples_map(*Pe, N_SI)
    for a in (*sysm, Y, Ye):
        a.setflags(write=False)
    return sysm, Y, Ye


def _raw(fb, w, channels, t_sim, dt, stride=1, want_y=True):
    """the C ABI itself: (y [ns, m, n] or None, info [9, m, n], status [m, n])"""
    iu = np.array([c[0] for c in channels], dtype=np.int32); iy = np.array([c[1] for c in channels], dtype=np.int32)
    m, n = len(channels), w.n
    y = np.full((fb.timeresp.samples(int(round(t_sim / (dt if dt > 0 else w.Ts))), stride), m, n), np.nan) if want_y else None
    info, status = np.full((9, m, n), np.nan), np.full((m, n), -1, dtype=np.int32)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = fb.lib.fb_lss_stepinfo(w._h, iu.ctypes.data_as(C.POINTER(C.c_int32)), iy.ctypes.data_as(C.POINTER(C.c_int32)), m, t_sim, dt, None, None, None,
                                stride, pd(y), pd(info), status.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, fb.lib.fb_last_error()
    return y, info, status


@pytest.mark.parametrize("nx", tr.NX_ALL)
def test_sampled_stepinfo_against_the_exact_samples(fb, nx, capsys):
    sysm, Y, Ye = _si_reference(nx)
    n, m = tr.N_SYS, len(tr.CHANNELS)
    cont = fb.LinearWorld(tr.model(fb, *sysm))
    rk4_raw = _raw(fb, cont, tr.CHANNELS, tr.T_SIM, tr.DT)          # before anything of the new path has run on this world
    res = fb.c2d(cont, proto.SI_TS)
    assert res.ok.all()
    w = res.world
    r = fb.timeresp.step(w, tr.CHANNELS, proto.SI_TSIM)
    assert r.y.shape == (n, m, N_SI + 1) and r.t[-1] == N_SI * proto.SI_TS and (r.status == 0).all() and r.c2d_status is None
    Yd = r.y.transpose(2, 1, 0).reshape(N_SI + 1, m * n)
    d, p = tr.sample_dev(Yd, Ye), tr.sample_dev(Y, Ye)
    with capsys.disabled():
        print(f"\n[fb_lss_stepinfo on a sampled world vs exact] nx {nx:2d}, {n} x {m}, N {N_SI}: samples {d.max():.2e} of max|y| (prototype {p.max():.2e}; "
              f"device vs prototype {tr.sample_dev(Yd, Y).max():.2e})", end="")
    assert d.max() <= max(MARGIN * p.max(), FLOOR)
    zoh = fb.timeresp.step(cont, tr.CHANNELS, proto.SI_TSIM, dt=proto.SI_TS, method="zoh")
    assert _same(zoh.y, r.y) and np.array_equal(zoh.c2d_status, np.zeros(n, dtype=np.int32))
    P = tr.pairs(*sysm, tr.CHANNELS)
    for name, (y0_in, yf_in, opts) in tr.gpu_variants(P, Ye).items():
        shape = lambda a: None if a is None else a.reshape(m, n).T
        si = fb.stepinfo(w, tr.CHANNELS, proto.SI_TSIM, y0=shape(y0_in), yf=shape(yf_in), settling_th=opts[0], risetime_th=opts[1:])
        info = np.array([getattr(si, f).T.reshape(-1) for f in tr.FIELDS])
        info_p, st_p = tr.stepinfo_batch(Y, proto.SI_TS, y0_in, yf_in, opts)
        assert (si.status == 0).all() and si.ok.all() and (st_p == 0).all() and si.dt == proto.SI_TS
        for k in (4, 7, 8):
            assert np.array_equal(info[k], info_p[k], equal_nan=True), (name, tr.FIELDS[k])
        si2 = fb.stepinfo(cont, tr.CHANNELS, proto.SI_TSIM, dt=proto.SI_TS, y0=shape(y0_in), yf=shape(yf_in), settling_th=opts[0], risetime_th=opts[1:],
                          method="zoh")
        assert all(_same(getattr(si, f), getattr(si2, f)) for f in tr.FIELDS) and si2.ok.all() and (si2.c2d_status == 0).all()
    # method="rk4" (the default) on the same world: the bits of the call made before c2d ran, and of the C ABI now
    rk4 = fb.timeresp.step(cont, tr.CHANNELS, tr.T_SIM, dt=tr.DT)
    again = _raw(fb, cont, tr.CHANNELS, tr.T_SIM, tr.DT)
    assert _same(rk4.y.transpose(2, 1, 0), rk4_raw[0]) and _same(again[0], rk4_raw[0]) and _same(again[1], rk4_raw[1]) and rk4.c2d_status is None
    assert not _same(rk4.y, r.y)
    w.close()
    cont.close()


def test_sampled_stepinfo_strides_and_no_sample_buffer(fb):
    sysm = _si_reference(8)[0]
    cont = fb.LinearWorld(tr.model(fb, *sysm))
    w = fb.c2d(cont, proto.SI_TS).world
    y1, info1, st1 = _raw(fb, w, tr.CHANNELS, proto.SI_TSIM, proto.SI_TS)
    assert y1.shape[0] == N_SI + 1 and not np.isnan(y1).any() and (st1 == 0).all()
    for dt in (0.0, np.nan):          # 0 or a non-finite dt: the world's own Ts
        y, info, st = _raw(fb, w, tr.CHANNELS, proto.SI_TSIM, dt)
        assert _same(y, y1) and _same(info, info1) and np.array_equal(st, st1)
    for stride in (7, N_SI, N_SI + 5):
        y, info, st = _raw(fb, w, tr.CHANNELS, proto.SI_TSIM, proto.SI_TS, stride=stride)
        rows = list(range(0, N_SI, stride)) + [N_SI]
        assert y.shape[0] == len(rows) == -(-N_SI // stride) + 1
        assert _same(y, y1[rows]) and _same(info, info1) and np.array_equal(st, st1), stride
        res = fb.timeresp.step(w, tr.CHANNELS, proto.SI_TSIM, stride=stride)
        assert np.array_equal(res.t, np.array(rows) * proto.SI_TS) and _same(res.y.transpose(2, 1, 0), y)
    _, info, st = _raw(fb, w, tr.CHANNELS, proto.SI_TSIM, proto.SI_TS, want_y=False)
    assert _same(info, info1) and np.array_equal(st, st1)
    w.close()
    cont.close()


# ---- 8. the notebook's two tables ------------------------------------------------------------------------------------------------------------------------------
def test_the_notebooks_tables_with_zoh(fb, capsys):
    tables = tr.stored_tables()
    loops = dict(zip(("velocity_loop", "position_loop"), tr.notebook_loops_from_golden()))
    labels = {"velocity_loop": ("v_ref", "v"), "position_loop": ("η_ref", "η")}
    for which, (Al, b, c, d) in loops.items():
        t = tables[which]
        cw = fb.LinearWorld(tr.loop_model(fb, Al, b, c, d, labels=labels[which]))
        si = fb.stepinfo(cw, [labels[which]], t["t_sim"], dt=t["dt"], method="zoh")
        cw.close()
        text = si.show(0, 0)
        with capsys.disabled():
            print(f"\n[fb_lss_stepinfo, method zoh, Robot2D {which}] " + "; ".join(" ".join(s.split()) for s in text.split("\n")), end="")
        assert si.ok.all() and (si.c2d_status == 0).all() and si.dt == t["dt"]
        tr.assert_matches_table(text.split("\n"), which)


# ---- 9. lsim ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_lsim_on_the_demos_input(fb, capsys):
    n = 3
    ac = fb.BatchedWorld(n, kinematics="NED")
    lss = fb.linearize(ac, fb.TrimParameters(EAS=np.array([42.0, 46.0, 50.0]), h_e=np.array([600.0, 1200.0, 2000.0])))
    assert lss.success.all()
    w = fb.linear_world(ac, u=("elevator",), y=("q",))
    ac.close()
    t = np.arange(0, 10.005, 0.01)
    iu, iq = lss.u_labels.index("elevator"), lss.y_labels.index("q")
    u0 = lss.u0[:, iu:iu + 1]
    U = u0[None] + (0.1 * (t >= 1))[:, None, None]          # [nt, n, 1]: the demo's 0.1 (t >= 1) on top of the trim elevator
    before = (w.x, w.u, *clock(fb, w), *w.model())
    y, x = fb.lsim(w, U.transpose(0, 2, 1), t)
    after = (w.x, w.u, *clock(fb, w), *w.model())
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and w.Ts == 0.0
    A, B = w.model()
    Cm, D = w.model_cd()
    w.close()
    assert y.shape == (t.size, 1, n) and x.shape == (t.size, 16, n)
    Phi, Gam, dl = proto.exact_batch(A, B, lss.xdot0, 0.01)
    y0 = lss.y0[:, iq:iq + 1]
    ye, xe = proto.lsim(Phi, Gam, dl, Cm, D, lss.x0, u0, y0, lss.x0.copy(), U)
    dev = float(np.abs(y.transpose(0, 2, 1) - ye).max() / np.abs(ye).max())
    with capsys.disabled():
        print(f"\n[lsim, Cessna172Sv0 e2q, 0.1 (t >= 1) on 0:0.01:10] {n} aircraft: q {dev:.2e} of max|q| = {np.abs(ye).max():.3e} against the exact recursion",
              end="")
    assert dev <= 1e-11


def test_lsim_carries_the_new_input_at_a_change(fb):
    one = lambda v: np.array(v, dtype=np.float64)
    z = np.zeros((1, 1))
    m = fb.LinearizedSS(xdot0=z, x0=z, u0=z, y0=z, A=one([[[-1.0]]]), B=one([[[1.0]]]), C=one([[[1.0]]]), D=one([[[10.0]]]), x_labels=("x",),
                        u_labels=("u",), y_labels=("y",))
    w = fb.LinearWorld(m)
    t = 0.1 * np.arange(6)
    u = one([0, 0, 1, 1, 0.5, 0.5])
    y, x = fb.lsim(w, u, t)
    Phi, Gam, dl = proto.exact_batch(m.A, m.B, m.xdot0, t[1] - t[0])
    ye, xe = proto.lsim(Phi, Gam, dl, m.C, m.D, z, z, z, z.copy(), u.reshape(6, 1, 1))
    assert y.shape == (6, 1, 1) and x.shape == (6, 1, 1)
    assert y[:3, 0, 0].tolist() == [0.0, 0.0, 10.0] and x[:3, 0, 0].tolist() == [0.0, 0.0, 0.0]          # the sample AT the change carries the new input
    assert np.abs(y[:, 0, 0] - ye[:, 0, 0]).max() <= 1e-11 * np.abs(ye).max() and np.abs(x[:, 0, 0] - xe[:, 0, 0]).max() <= 1e-11
    s = fb.c2d(w, t[1] - t[0]).world          # a sampled world passed in directly, per-system inputs, a given x0
    y2, x2 = fb.lsim(s, u.reshape(6, 1, 1), t, x0=[0.0])
    assert _same(y2, y) and _same(x2, x)
    with pytest.raises(fb.FlightBatchError, match="sampled at Ts"):
        fb.lsim(s, u, 2 * t)
    s.close()
    w.close()


# ---- 10. refusals on a live device -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 4
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def refused(h, cause, call, name=b""):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        rc = call()
        err = fb.lib.fb_last_error()
        assert rc != 0 and cause in err and name in err and launches(h) == 0, (cause, err)

    def c2d(h, Ts=0.01, out=True):
        o = C.c_void_p()
        rc = fb.lib.fb_lss_c2d(h, Ts, None, None, C.byref(o) if out else None)
        assert not o.value or rc == 0
        if o.value:
            fb.lib.fb_destroy(o)
        return rc

    M = proto.plants(3, 2, n)
    w = fb.LinearWorld(proto.model(fb, M))
    r = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(r._h, b"not a LinearizedSS handle", lambda: c2d(r._h), b"fb_lss_c2d")
    ts = C.c_double()
    refused(r._h, b"not a LinearizedSS handle", lambda: fb.lib.fb_lss_sample_time(r._h, C.byref(ts)), b"fb_lss_sample_time")
    r.close()
    refused(w._h, b"Ts is null", lambda: fb.lib.fb_lss_sample_time(w._h, None), b"fb_lss_sample_time")
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 3, n, 0, C.byref(h)) == 0
    refused(h, b"no model yet", lambda: c2d(h), b"fb_lss_c2d")
    fb.lib.fb_destroy(h)
    for Ts in (0.0, -0.01, np.inf, np.nan):
        refused(w._h, b"must be positive and finite", lambda: c2d(w._h, Ts), b"fb_lss_c2d")
    refused(w._h, b"out is null", lambda: c2d(w._h, out=False), b"fb_lss_c2d")
    assert fb.lib.fb_timing_begin_per_launch(w._h, 8) == 0
    res = fb.c2d(w, 0.01)
    assert launches(w._h) == 1 and res.ok.all()          # the kernel runs on the source's stream, where its stamps are
    s = res.world
    verb = b"a continuous-time verb on a sampled model"
    refused(s._h, b"itself a sampled model", lambda: c2d(s._h), b"fb_lss_c2d")
    b8 = [np.zeros(64) for _ in range(8)]
    refused(s._h, b"sampled model", lambda: fb.lib.fb_lss_set_model(s._h, *[pd(a) for a in b8]), b"fb_lss_set_model")
    xd = np.empty((3, n))
    refused(s._h, b"no derivative", lambda: fb.lib.fb_f_ode(s._h, pd(xd)), b"fb_f_ode")
    info, st = np.empty((9, 1, n)), np.empty((1, n), dtype=np.int32)
    ch = np.zeros(1, dtype=np.int32)
    refused(s._h, b"on a sampled model with Ts", lambda: fb.lib.fb_lss_stepinfo(s._h, pi(ch), pi(ch), 1, 1.0, 0.02, None, None, None, 1, None, pd(info), pi(st)),
            b"fb_lss_stepinfo")
    s.set_params(dt=0.02)
    refused(s._h, b"steps by its own sample time only", lambda: fb.lib.fb_step(s._h, 1), b"fb_step")
    s.set_params(dt=0.01)
    refused(s._h, verb, lambda: fb.lib.fb_lqr(s._h, None, None, None, None, None, None, None), b"fb_lqr")
    refused(s._h, verb, lambda: fb.lib.fb_pid_metrics(s._h, 0, 0, None, 0, 1.0, 0.01, None, None, 0, None, None, None), b"fb_pid_metrics")
    refused(s._h, verb, lambda: fb.lib.fb_lss_freqresp(s._h, 0, 0, None, 0, None, None), b"fb_lss_freqresp")
    refused(s._h, verb, lambda: fb.lib.fb_lss_poles(s._h, None, None, None, None), b"fb_lss_poles")
    o = C.c_void_p()
    refused(s._h, verb, lambda: fb.lib.fb_lss_connect(s._h, None, None, 0, None, 0, None, 0, 0, None, 0, None, C.byref(o)), b"fb_lss_connect")
    refused(w._h, verb, lambda: fb.lib.fb_lss_connect(w._h, s._h, None, 0, None, 0, None, 0, 0, None, 0, None, C.byref(o)), b"fb_lss_connect")
    refused(s._h, verb, lambda: fb.lib.fb_lss_transform(s._h, None, None, None, 0, None, 0, None, 0, None, None, C.byref(o)), b"fb_lss_transform")
    refused(s._h, verb, lambda: fb.lib.fb_lss_steady(s._h, None, 0, None, 0, None, None, None, None, None), b"fb_lss_steady")
    assert not o.value
    with pytest.raises(fb.FlightBatchError, match="a continuous-time verb on a sampled model"):
        fb.poles(s)
    with pytest.raises(ValueError, match='"rk4" or "zoh"'):
        fb.timeresp.step(w, [(0, 0)], 1.0, dt=0.01, method="tustin")
    # what still works on the sampled handle: the outputs, the model, the step
    s.f_ode()
    assert _same(s.y.T, M[3]) and _same(s.model_cd()[0], M[6]) and s.Ts == 0.01
    s.close()
    w.close()
