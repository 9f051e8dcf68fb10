"""fb_lss_dconnect (flightbatch.dconnect): two batches of SAMPLED linear models connected through static gains and unit delays on the device,
pinned by

  1. the longdouble restatement (tests/dconnect_prototype.py) on nine shapes x N in {1, 63, 130}: the extended state at both edges of every
     group size of the kernel;
  2. the closed form of 1 / (z - 1) read one sample late, to the bit, with dpoles and dmargins of the result;
  3. a delay that breaks an algebraic loop, an ill-posed and a non-finite system flagged in place among healthy ones;
  4. nd = 0 against fb_lss_connect on the same four matrices, bit for bit;
  5. position independence and reproducibility, bit for bit, and the sources left as they were;
  6. the new handle as an ordinary sampled one: stepped by fb_step and sampled by timeresp.step against a tick-by-tick simulation of the
     interconnection, reloaded from its matrices, connected again;
  7. the device's other verbs: dlqr's closed world, dpoles of a delayed state feedback, the flown PID law closed by dunity_feedback against
     dpid_metrics, dseries with a delay through dfreqresp;
  8. the refusals of the C ABI on a live device.

The bound of 1 is the family's rule (tests/test_gpu_connect.py): the device differs from the float64 restatement in FMA contraction, in the
term a sum starts from and in <= 1-ulp division only, so its deviation from the longdouble side may be ten times the prototype's over the
same systems, with 1e-13 as the floor. A deviation is max|got - want| over a block divided by the block's largest |want|, per system, the
worst over the batch; a block whose largest |want| is 0 is held to equality. The stepping bound of 6 is ten times the deviation
tests/test_dconnect_host.py prints for the shape (the float64 restatement against the same simulation), with 1e-11 as the floor."""
import ctypes as C
import functools

import numpy as np
import pytest

import dconnect_prototype as proto
import dmargins_prototype as dm
import dpid_prototype as dpp
from support import clock

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-13, 10.0
STEP_FLOOR = 1e-11
BLOCKS = ("Phi'", "Gamma'", "C'", "D'")
TS = 0.02
MID = (9, 1, 4, 1, 20, 1, 7, 16, 4, 21)
SMALL = (5, 1, 2, 1, 3, 1, 3, 2, 2, 4)
pi32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
same = lambda a, b: np.array_equal(a, b, equal_nan=True)


def _lss(fb, side, tag, seed):
    """a side (Phi, Gamma, C, D) [n, ., .] as a LinearizedSS whose delta, x0, u0, y0 are random numbers (they play no part)"""
    A, B, Cm, D = side
    n, nx, nu, ny = A.shape[0], A.shape[1], B.shape[2], Cm.shape[1]
    rng = np.random.default_rng(seed)
    return fb.LinearizedSS(xdot0=rng.standard_normal((n, nx)), x0=rng.standard_normal((n, nx)), u0=rng.standard_normal((n, nu)),
                           y0=rng.standard_normal((n, ny)), A=A, B=B, C=Cm, D=D, x_labels=tuple(f"x{tag}{k}" for k in range(nx)),
                           u_labels=tuple(f"u{tag}{k}" for k in range(nu)), y_labels=tuple(f"y{tag}{k}" for k in range(ny)))


def _take(side, keep):
    return None if side is None else tuple(np.ascontiguousarray(m[keep]) for m in side)


def _worlds(fb, P, Cc, Ts=TS):
    return fb.LinearWorld(_lss(fb, P, "p", 1), Ts=Ts), (fb.LinearWorld(_lss(fb, Cc, "c", 2), Ts=Ts) if Cc is not None else None)


def _read(res, close=True):
    w = res.world
    out = w.model() + w.model_cd() + (res.status.copy(),)
    if close:
        w.close()
    return out


def _dconnect(fb, cs, keep=slice(None), batch_wide=None):
    """(Phi', Gamma', C', D', status) of the systems `keep` of a case; batch_wide = i: system i's F and G for the whole batch, as [nv, .] matrices"""
    P, Cc, dz, jz, F, G, iz = cs
    pw, cw = _worlds(fb, _take(P, keep), _take(Cc, keep))
    Fk, Gk = (F[keep], G[keep]) if batch_wide is None else (F[batch_wide], G[batch_wide])
    res = fb.dconnect(pw, cw, feedback=Fk, inputs=Gk, delays=dz, reads=jz, outputs=iz)
    nx = P[0].shape[1] + (Cc[0].shape[1] if Cc else 0) + len(dz)
    assert res.world.n == pw.n and (res.world.nx, res.world.nu, res.world.ny) == (nx, G.shape[2], len(iz)) and res.world.Ts == TS
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


def _launches(fb, h):
    ms, nl = C.c_float(), C.c_int64()
    assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
    assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
    return nl.value


# ---- 1. accuracy -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("shape", proto.SHAPES, ids=proto.ident)
def test_against_the_longdouble_side(fb, shape, n, capsys):
    cs, f64, long = proto.sides(shape)
    got = _dconnect(fb, cs, slice(0, n))
    assert (got[4] == 0).all() and (f64[4] == 0).all()
    _hold(f"fb_lss_dconnect {proto.ident(shape)} N {n}", got[:4], [m[:n] for m in long[:4]], [m[:n] for m in f64[:4]], capsys)


# ---- 2. the closed form ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nxe", [2, 8, 9, 16, 17, 32])
def test_the_delayed_integrator_loop_to_the_bit(fb, nxe, capsys):
    """1 / (z - 1) among decoupled stable states (nx' = nxe), its output read one sample late, v = -K q + K w:
    Phi' = [[1, -K], [1, 0]], Gamma' = [K, 0]', C' = [1, 0] among the untouched states; stable exactly for K < 1; the open loop w -> q is
    K / (z (z - 1)) with GM = 1 / K"""
    Ks = np.array([0.25, 0.5, 2.0, 0.25, 0.5, 2.0, 0.5])
    n, nx = Ks.size, nxe - 1
    rng = np.random.default_rng(100 + nxe)
    Phi = np.zeros((n, nx, nx))
    for i in range(n):
        Phi[i] = np.diag(np.concatenate([[1.0], rng.integers(-7, 8, nx - 1) / 8.0]))
    Gam = np.zeros((n, nx, 1)); Gam[:, 0, 0] = 1.0
    Cm = np.zeros((n, 1, nx)); Cm[:, 0, 0] = 1.0
    pw, _ = _worlds(fb, (Phi, Gam, Cm, np.zeros((n, 1, 1))), None)
    res = fb.dconnect(pw, feedback=-Ks.reshape(n, 1, 1), inputs=Ks.reshape(n, 1, 1), delays=[0], reads=["yp0[k-1]"], outputs=["yp0"])
    assert res.ok.all() and res.world.x_labels == pw.x_labels + ("yp0[k-1]",) and res.world.y_labels == ("yp0",) and res.world.Ts == TS
    P1, G1, C1, D1, _ = _read(res, close=False)
    wantP = np.zeros((n, nxe, nxe)); wantP[:, :nx, :nx] = Phi; wantP[:, 0, nx] = -Ks; wantP[:, nx, 0] = 1.0
    wantG = np.zeros((n, nxe, 1)); wantG[:, 0, 0] = Ks
    wantC = np.zeros((n, 1, nxe)); wantC[:, 0, 0] = 1.0
    assert np.array_equal(P1, wantP) and np.array_equal(G1, wantG) and np.array_equal(C1, wantC) and not D1.any()
    lam = fb.dpoles(res.world)
    assert (lam.status == 0).all() and lam.stable.tolist() == (Ks < 1.0).tolist()
    res.world.close()
    # the open loop w -> q: nothing is fed back (F = 0 on the delayed read), the input gain is K, the output is the delayed row
    opn = fb.dconnect(pw, feedback=np.zeros((1, 1)), inputs=Ks.reshape(n, 1, 1), delays=["yp0"], reads=[1], outputs=[1])
    assert opn.ok.all() and opn.world.y_labels == ("yp0[k-1]",)
    mg = fb.dmargins(opn.world, "w0", "yp0[k-1]", dm.W_CLOSED)
    dev_d = dev_p = 0.0
    for i, K in enumerate(Ks):
        Po = np.zeros((nxe, nxe)); Po[:nx, :nx] = Phi[i]; Po[nx, 0] = 1.0
        g = np.zeros(nxe); g[0] = K
        c = np.zeros(nxe); c[nx] = 1.0
        pr = dm.margins(Po, g, c, 0.0, dm.W_CLOSED, TS)
        dev_d, dev_p = max(dev_d, abs(mg.gm[i] * K - 1.0)), max(dev_p, abs(pr[0][0] * K - 1.0))
    with capsys.disabled():
        print(f"\n[dconnect, K / (z (z - 1)) at nx' = {nxe}] GM K - 1: device {dev_d:.2e}, prototype {dev_p:.2e}", end="")
    assert (mg.status == 0).all() and dev_d <= max(dm.FACTOR * dev_p, dm.FLOOR)
    opn.world.close(); pw.close()


# ---- 3. a delay breaks the algebraic loop; failures in place -----------------------------------------------------------------------------------------
def test_a_delay_breaks_the_algebraic_loop_and_failures_stay_in_place(fb):
    """one-state plants with D = 1; the feedback reads the output now (F[:, 0]) and one sample late (F[:, 1]). F = (1, 0): 1 - F D = 0, ill-posed;
    F = (0, 1): the same gain on the delayed read, well-posed; a NaN in F: not finite; 63 healthy systems around them"""
    n, bad, late, nanf = 66, 17, 40, 64
    rng = np.random.default_rng(23)
    P = (rng.uniform(-0.9, 0.9, (n, 1, 1)), rng.standard_normal((n, 1, 1)), rng.standard_normal((n, 1, 1)), np.ones((n, 1, 1)))
    F = rng.uniform(-0.5, 0.5, (n, 1, 2))
    F[bad] = [[1.0, 0.0]]; F[late] = [[0.0, 1.0]]; F[nanf, 0, 1] = np.nan
    G = rng.standard_normal((n, 1, 1))
    cs = (P, None, np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), F, G, np.array([1, 0], dtype=np.int32))
    got = _dconnect(fb, cs)
    expect = np.zeros(n, dtype=np.int32); expect[bad] = fb.K["FB_CONNECT_ILL_POSED"]; expect[nanf] = fb.K["FB_CONNECT_NOT_FINITE"]
    assert np.array_equal(got[4], expect), got[4]
    for m in got[:4]:
        assert np.isnan(m[bad]).all() and np.isnan(m[nanf]).all() and np.isfinite(m[late]).all()
    pro = proto.dconnect_batch(*cs)
    assert np.array_equal(pro[4], expect)
    # the delayed read: Phi' = [[Phi, Gamma], [C, 1]], Gamma' = [Gamma g; g] (every pivot is 1: the products are exact, the sums have one term)
    assert np.array_equal(got[0][late], pro[0][late]) and np.array_equal(got[1][late], pro[1][late])
    assert np.array_equal(got[0][late], [[P[0][late, 0, 0], P[1][late, 0, 0]], [P[2][late, 0, 0], 1.0]])
    healthy = np.flatnonzero((expect == 0) & (np.arange(n) != late))
    assert healthy.size == 63
    ref = _dconnect(fb, cs, healthy)
    assert (ref[4] == 0).all() and all(same(a[healthy], b) and np.isfinite(b).all() for a, b in zip(got[:4], ref[:4]))
    # with nd = 0 the same system under F = 1 on its own output is ill-posed
    one = _take(P, slice(bad, bad + 1))
    now = _dconnect(fb, (one, None, np.zeros(0, dtype=np.int32), np.array([0], dtype=np.int32), np.ones((1, 1, 1)), G[bad:bad + 1], np.array([0], dtype=np.int32)))
    assert now[4][0] == fb.K["FB_CONNECT_ILL_POSED"] and all(np.isnan(m).all() for m in now[:4])


# ---- 4. nd = 0 is connect ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(15, 1, 4, 1, 33, 1, 0, 16, 4, 34), (4, 1, 1, 1, 6, 1, 0, 4, 1, 7)], ids=proto.ident)
def test_without_a_delay_the_bits_are_connects(fb, shape):
    P, Cc, dz, jz, F, G, iz = proto.case(shape)
    assert dz.size == 0
    pc, cc = fb.LinearWorld(_lss(fb, P, "p", 1)), fb.LinearWorld(_lss(fb, Cc, "c", 2))
    cont = _read(fb.connect(pc, cc, feedback=F, inputs=G, reads=jz, outputs=iz))
    pc.close(); cc.close()
    samp = _dconnect(fb, (P, Cc, dz, jz, F, G, iz))
    assert (cont[4] == 0).all() and np.isfinite(cont[0]).all() and cont[0].any()
    assert all(same(a, b) for a, b in zip(cont, samp))


# ---- 5. bit for bit ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid(fb):
    out = _dconnect(fb, proto.sides(MID)[0])
    for a in out:
        a.setflags(write=False)
    return out


def test_a_second_call_and_the_batch_in_another_order(fb):
    cs = proto.sides(MID)[0]
    full = _mid(fb)
    assert (full[4] == 0).all()
    again = _dconnect(fb, cs)
    assert all(same(a, b) for a, b in zip(full, again))
    rev = _dconnect(fb, cs, slice(None, None, -1))
    assert all(same(a, b[::-1]) for a, b in zip(full, rev))
    keep = np.array([129, 3, 64, 63, 0, 77, 12])
    sub = _dconnect(fb, cs, keep)
    assert all(same(a[keep], b) for a, b in zip(full, sub))
    for n in (1, 63):
        head = _dconnect(fb, cs, slice(0, n))
        assert all(same(a[:n], b) for a, b in zip(full, head))


def test_batch_wide_gains_are_the_replicated_ones(fb):
    P, Cc, dz, jz, F, G, iz = proto.sides(MID)[0]
    n = 63
    rep = (_take(P, slice(0, n)), _take(Cc, slice(0, n)), dz, jz, np.repeat(F[5:6], n, axis=0), np.repeat(G[5:6], n, axis=0), iz)
    per = _dconnect(fb, rep)
    wide = _dconnect(fb, (P, Cc, dz, jz, F, G, iz), slice(0, n), batch_wide=5)
    assert (per[4] == 0).all() and all(same(a, b) for a, b in zip(per, wide))


def test_the_sources_are_left_as_they_were(fb):
    P, Cc, dz, jz, F, G, iz = proto.sides(MID)[0]
    pw, cw = _worlds(fb, P, Cc)
    rng = np.random.default_rng(8)
    for w in (pw, cw):
        w.u = rng.standard_normal((w.nu, w.n))
    pw.log_configure(every=2, capacity=8, y=[0, 1], x=[0])
    pw.step(7)
    pw.sync()

    def snapshot(w):
        t, data = w.log_read() if w is pw else (np.zeros(0), np.zeros(0))
        return (w.x, w.u, w.status, np.array(clock(fb, w)), np.array(w.Ts), t, data) + w.model() + w.model_cd()
    before = [snapshot(w) for w in (pw, cw)]
    res = fb.dconnect(pw, cw, feedback=F, inputs=G, delays=dz, reads=jz, outputs=iz)
    after = [snapshot(w) for w in (pw, cw)]
    for b, a in zip(before, after):
        assert all(same(x, y) for x, y in zip(b, a))
    assert clock(fb, pw) == (pytest.approx(7 * TS), 7) and not before[0][2].any() and pw.Ts == cw.Ts == TS
    # the new handle: sampled with p's Ts, at rest, clock at zero
    w = res.world
    assert w.Ts == TS and clock(fb, w) == (0.0, 0) and not w.x.any() and not w.u.any() and (w.status == 0).all()
    w.step(1)
    w.sync()
    assert clock(fb, w) == (pytest.approx(TS), 1)
    assert all(same(a, b) for a, b in zip(_read(res), _mid(fb)))
    pw.close(); cw.close()


# ---- 6. an ordinary sampled handle ---------------------------------------------------------------------------------------------------------------------
def _step_bound(shape):
    w, ref, got = proto.tick_sides(shape)
    return max(MARGIN * float(proto.run_dev(got, ref).max()), STEP_FLOOR)


def test_the_new_handle_steps_as_the_interconnection_does(fb, capsys):
    shape = MID          # (the mildest growth over 50 ticks among the shapes: the random loops are not stable)
    P, Cc, dz, jz, F, G, iz = proto.sides(shape)[0]
    n, nw, ny = 63, shape[8], shape[9]
    take = lambda S, i: tuple(m[i] for m in S)
    pw, cw = _worlds(fb, _take(P, slice(0, n)), _take(Cc, slice(0, n)))
    res = fb.dconnect(pw, cw, feedback=F[:n], inputs=G[:n], delays=dz, reads=jz, outputs=iz)
    a = res.world
    assert res.ok.all() and a.Ts == TS
    ts = C.c_double(-1.0)
    assert fb.lib.fb_lss_sample_time(a._h, C.byref(ts)) == 0 and ts.value == pw.Ts == TS
    Phi, Gam = a.model()
    Cm, D = a.model_cd()
    z = np.zeros
    b = fb.LinearWorld(fb.LinearizedSS(xdot0=z((n, a.nx)), x0=z((n, a.nx)), u0=z((n, a.nu)), y0=z((n, a.ny)), A=Phi, B=Gam, C=Cm, D=D,
                                       x_labels=a.x_labels, u_labels=a.u_labels, y_labels=a.y_labels), Ts=TS)
    bound = _step_bound(shape)
    u = np.random.default_rng(11).standard_normal((nw, n))
    nsteps = 50
    want = np.array([proto.simulate(take(P, i), take(Cc, i), dz, jz, F[i], G[i], iz, np.repeat(u[None, :, i], nsteps + 1, axis=0))[nsteps] for i in range(n)])
    for spl in (1, 7, 50):
        outs = []
        for w in (a, b):
            w.set_state(z((w.nx, n)))
            w.u = u
            assert fb.lib.fb_set_steps_per_launch(w._h, spl) == 0
            w.step(nsteps)
            w.sync()
            w.f_ode()
            outs.append((w.x, w.y, np.array(clock(fb, w))))
        assert all(same(p, q) for p, q in zip(*outs)) and clock(fb, a) == (pytest.approx(nsteps * TS), nsteps)
        y = outs[0][1].T
        dev = float((np.abs(y - want).max(axis=1) / np.abs(want).max(axis=1)).max())
        with capsys.disabled():
            print(f"\n[dconnect {proto.ident(shape)}, {nsteps} steps of fb_step at {spl} per launch vs the tick-by-tick simulation] {dev:.2e} (bound {bound:.2e})", end="")
        assert np.isfinite(y).all() and y.any() and dev <= bound
    # timeresp.step samples the same map: a unit step on input j, output k, ticks 0 .. 12
    nt = proto.TICKS
    nk = 4               # (the first outputs: a call takes at most 64 channels)
    sr = fb.timeresp.step(a, [(j, k) for j in range(nw) for k in range(nk)], nt * TS)
    assert (sr.status == 0).all() and sr.y.shape == (n, nw * nk, nt + 1)
    worst = 0.0
    for i in range(n):
        for j in range(nw):
            w1 = np.zeros((nt + 1, nw)); w1[:, j] = 1.0
            ref = proto.simulate(take(P, i), take(Cc, i), dz, jz, F[i], G[i], iz, w1)[:, :nk]          # [T, nk]
            got = sr.y[i, j * nk:(j + 1) * nk].T
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    with capsys.disabled():
        print(f"\n[dconnect {proto.ident(shape)}, timeresp.step vs the tick-by-tick simulation] {worst:.2e} (bound {bound:.2e})", end="")
    assert worst <= bound
    for w in (a, b, pw, cw):
        w.close()


def test_a_second_dconnect_makes_a_two_sample_delay(fb, capsys):
    """the result of one call is the plant of the next: z[r] delayed twice, fed back and put out, against the prototype applied twice"""
    shape = SMALL
    P, Cc, dz, jz, F, G, iz = proto.sides(shape)[0]
    n = 63
    pw, cw = _worlds(fb, _take(P, slice(0, n)), _take(Cc, slice(0, n)))
    nz = shape[4] + shape[5]
    # first call: delay row 1 of z, no feedback through it yet (F1 reads it with zeros), outputs every row of [z; q], inputs v itself
    nv = shape[2] + shape[3]
    one = fb.dconnect(pw, cw, feedback=np.zeros((nv, 1)), inputs=np.eye(nv), delays=[1], reads=[nz])
    assert one.ok.all() and one.world.ny == nz + 1 and one.world.y_labels[-1] == "yp1[k-1]"
    rng = np.random.default_rng(31)
    F2 = 0.3 * rng.standard_normal((n, nv, 2))
    G2 = rng.standard_normal((n, nv, 2))
    two = fb.dconnect(one.world, feedback=F2, inputs=G2, delays=["yp1[k-1]"], reads=["yp1[k-1][k-1]", "yp0"], outputs=["yp1", "yp1[k-1]", "yp1[k-1][k-1]"])
    assert two.ok.all() and two.world.nx == shape[0] + shape[1] + 2 and two.world.x_labels[-2:] == ("yp1[k-1]", "yp1[k-1][k-1]") and two.world.Ts == TS
    got = _read(two)
    sides = []
    for dtype in (np.float64, np.longdouble):
        first = proto.dconnect_batch(_take(P, slice(0, n)), _take(Cc, slice(0, n)), [1], [nz], np.zeros((nv, 1)), np.eye(nv), None, dtype)
        sides.append(proto.dconnect_batch(first[:4], None, [nz], [nz + 1, 0], F2, G2, [1, nz, nz + 1], dtype))
    assert (sides[0][4] == 0).all()
    _hold("a second fb_lss_dconnect on the result (a two-sample delay)", got[:4], sides[1][:4], sides[0][:4], capsys)
    for w in (one.world, pw, cw):
        w.close()


# ---- 7. against the device's other verbs ---------------------------------------------------------------------------------------------------------------
def _sampled_design(fb, n=9, nx=6, nu=2, seed=17):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, nx, nx)) - 1.5 * np.eye(nx)
    m = fb.design_model(A, rng.standard_normal((n, nx, nu)))
    cw = fb.LinearWorld(m)
    sw = fb.c2d(cw, TS)
    cw.close()
    assert sw.ok.all()
    return sw.world


def test_dstate_feedback_is_dlqrs_closed_world(fb, capsys):
    sw = _sampled_design(fb)
    nx, nu, n = sw.nx, sw.nu, sw.n
    des = fb.dlqr(sw, np.eye(nx), np.eye(nu), closed=True)
    assert (des.status == 0).all()
    res = fb.dstate_feedback(sw, des.K)
    assert res.ok.all() and res.world.Ts == TS and res.world.x_labels == sw.x_labels == res.world.y_labels and res.world.u_labels == sw.u_labels
    got = _read(res)
    closed = des.world.model() + des.world.model_cd()
    des.world.close()
    Phi, Gam = sw.model()
    Cm, D = sw.model_cd()
    args = ((Phi, Gam, Cm, D), None, [], list(range(nx)), -des.K, np.eye(nu), None)
    pro, long = proto.dconnect_batch(*args), proto.dconnect_batch(*args, dtype=np.longdouble)
    assert not got[3].any() and not closed[3].any()
    _hold("dstate_feedback with dlqr's K", got[:3], long[:3], pro[:3], capsys)
    _hold("dlqr(closed=True)'s world", closed[:3], long[:3], pro[:3], capsys)
    # delay=True: the control computed from x_k acts at tick k + 1; the poles are those of the host-assembled loop [[Phi, -Gamma K], [I, 0]]
    dl = fb.dstate_feedback(sw, des.K, delay=True)
    assert dl.ok.all() and dl.world.nx == 2 * nx and dl.world.ny == nx and dl.world.x_labels == sw.x_labels + tuple(f"{s}[k-1]" for s in sw.x_labels)
    lam = fb.dpoles(dl.world)
    assert (lam.status == 0).all()
    worst = 0.0
    for i in range(n):
        M = np.zeros((2 * nx, 2 * nx)); M[:nx, :nx] = Phi[i]; M[:nx, nx:] = -Gam[i] @ des.K[i]; M[nx:, :nx] = np.eye(nx)
        ev = np.linalg.eigvals(M)
        dist = np.abs(lam.poles[i][:, None] - ev[None, :])
        worst = max(worst, float(max(dist.min(axis=1).max(), dist.min(axis=0).max()) / max(1.0, np.linalg.norm(M, 2))))
    with capsys.disabled():
        print(f"\n[dstate_feedback(delay=True), dpoles vs LAPACK on the host-assembled loop] Hausdorff distance {worst:.2e} of max(1, |M|)", end="")
    # both eigenvalue routines are backward stable (a perturbation of about 1e-15 |M|); the loop has nx - nu eigenvalues at 0, and a cluster of
    # m equal eigenvalues may move by the m-th root of the perturbation when it is defective: 1e-7 admits a double one, an error in the loop is of order 1
    assert worst <= 1e-7
    for w in (dl.world, sw):
        w.close()


def test_the_flown_pid_loop_by_dunity_feedback_against_dpid_metrics(fb, capsys):
    """the nx = 7 pairs of tests/test_gpu_dpid.py's closed-loop route: the loop closed on the device by dpid_world + dunity_feedback, stepped by
    timeresp.step and swept by dfreqresp, against the unbounded fb_lss_dpid_metrics; the host-assembled loop on the same pairs sets the bound"""
    nx, n, m = 7, 6, 2
    IU, IY = 1, 2
    N = int(round(dpp.T_SIM / dpp.TS))
    Phi, gam, c, d, P, _, _ = dpp.edge_reference(nx)
    rep = lambda a: np.repeat(a[:n], m, axis=0)
    pts = P[:n, :m].reshape(n * m, 4)
    rng = np.random.default_rng(5)
    B = rng.standard_normal((n * m, nx, 2)); B[:, :, IU] = rep(gam)
    Cm = rng.standard_normal((n * m, 3, nx)); Cm[:, IY, :] = rep(c)
    D = rng.standard_normal((n * m, 3, 2)); D[:, IY, IU] = rep(d)
    lss = _lss(fb, (rep(Phi), B, Cm, D), "p", 5)
    lss.u_labels, lss.y_labels = ("other", "u"), ("y0", "y1", "y")
    pw = fb.LinearWorld(lss, Ts=dpp.TS)
    met = fb.dpid_metrics(pw, pts[:, None, :], u=IU, y=IY, settings=fb.Settings(t_sim=dpp.T_SIM), w=dpp.W7())
    assert (met.status == 0).all()
    want = met.metrics[:, 0]
    cw = fb.dpid_world(pts, dpp.TS)
    loop = fb.dunity_feedback(pw, cw, "u", "y")
    assert loop.ok.all() and loop.world.nx == nx + 2 and loop.world.u_labels == ("y_ref",) and loop.world.y_labels == ("y0", "y1", "y", "u")

    def metrics_of(world, ref, e_channel):
        sr = fb.timeresp.step(world, [(ref, "y"), (ref, "u")], dpp.T_SIM)
        assert (sr.status == 0).all() and sr.y.shape == (n * m, 2, N + 1)
        S = e_channel(world)
        return np.array([dpp.host_metrics(sr.y[k, 0], sr.y[k, 1], S[:, k], N) for k in range(n * m)])
    dev_side = metrics_of(loop.world, "y_ref", lambda w: 1.0 - fb.dfreqresp(w, "y_ref", "y", dpp.W7()))      # e = r - y
    loops = [dpp.closed_loop(rep(Phi)[k], rep(gam)[k], rep(c)[k], rep(d)[k], fb.build_dpid(pts[k], dpp.TS)) for k in range(n * m)]
    nzl, z = nx + 2, np.zeros
    hl = fb.LinearWorld(fb.LinearizedSS(xdot0=z((n * m, nzl)), x0=z((n * m, nzl)), u0=z((n * m, 1)), y0=z((n * m, 3)), A=np.array([q[0] for q in loops]),
                                        B=np.array([q[1] for q in loops]), C=np.array([q[2] for q in loops]), D=np.array([q[3] for q in loops]),
                                        x_labels=tuple(f"z{k}" for k in range(nzl)), u_labels=("r",), y_labels=("y", "u", "e")), Ts=dpp.TS)
    host_side = metrics_of(hl, "r", lambda w: fb.dfreqresp(w, "r", "e", dpp.W7()))
    dd, dh = dpp.rel_dev(dev_side, want), dpp.rel_dev(host_side, want)
    with capsys.disabled():
        print("\n[dunity_feedback + timeresp.step + dfreqresp vs fb_lss_dpid_metrics, nx 7: device-closed (host-assembled)] "
              + "  ".join(f"{k} {a:.2e} ({b:.2e})" for k, a, b in zip(("Ms", "ie", "ef", "iu", "up"), dd, dh)), end="")
    for a, b in zip(dd, dh):
        assert a <= max(MARGIN * b, STEP_FLOOR), (dd, dh)
    for w in (hl, loop.world, cw, pw):
        w.close()


def test_dseries_with_a_delay_is_one_more_sample_of_phase(fb, capsys):
    nx, n = 7, 12
    Phi, gam, c, d, P, _, _ = dpp.edge_reference(nx)
    pw = fb.LinearWorld(_lss(fb, (Phi[:n], gam[:n, :, None], c[:n, None, :], d[:n].reshape(n, 1, 1)), "p", 9), Ts=dpp.TS)
    cw = fb.dpid_world(P[:n, 0], dpp.TS)
    w = dpp.W7()
    L = []
    for delay in (0, 1):
        s = fb.dseries(pw, cw, 0, 0, delay=delay)
        assert s.ok.all() and s.world.nx == nx + 2 + delay and s.world.u_labels == ("e",) and s.world.y_labels == ("yp0", "u")
        L.append(fb.dfreqresp(s.world, "e", "yp0", w))            # [nw, n]
        s.world.close()
    want = L[0] * np.exp(-1j * w * dpp.TS)[:, None]
    dev = float(np.abs(L[1] / want - 1.0).max())
    with capsys.disabled():
        print(f"\n[dseries(delay=1) through dfreqresp vs e^(-j w Ts) times delay=0's response] {dev:.2e}", end="")
    assert np.isfinite(L[0]).all() and dev <= dm.FLOOR          # (dfreqresp's floor, tests/test_gpu_dmargins.py: both sides are the device's)
    with pytest.raises(ValueError, match="delay = 2"):
        fb.dseries(pw, cw, 0, 0, delay=2)
    pw.close(); cw.close()


# ---- 8. refusals on a live device ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 5

    def lss(nx, nu, ny, nn=n, seed=0):
        return _lss(fb, tuple(np.random.default_rng(seed).standard_normal(s) for s in ((nn, nx, nx), (nn, nx, nu), (nn, ny, nx), (nn, ny, nu))), "p", 3)
    mk = lambda *a, Ts=TS, **k: fb.LinearWorld(lss(*a, **k), Ts=Ts)

    def call(p, c=None, dz=(), nd=None, jz=(0,), nf=None, F=True, G=True, nw=1, iz=(0,), ny=None, out=True, timed=True):
        if timed:
            assert fb.lib.fb_timing_begin_per_launch(p, 8) == 0
        cd_ = None if dz is None else np.array(dz, dtype=np.int32)
        cj = None if jz is None else np.array(jz, dtype=np.int32)
        ci = None if iz is None else np.array(iz, dtype=np.int32)
        buf = np.zeros(16 * 32 * 8)
        h = C.c_void_p(1)
        rc = fb.lib.fb_lss_dconnect(p, c, pi32(cd_), (len(dz) if dz is not None else 0) if nd is None else nd, pi32(cj), len(jz) if nf is None else nf,
                                    pd(buf) if F else None, 0, pd(buf) if G else None, 0, nw, pi32(ci),
                                    (len(iz) if iz is not None else 0) if ny is None else ny, None, C.byref(h) if out else None)
        err = fb.lib.fb_last_error()
        if rc == 0:
            fb.lib.fb_destroy(h)
        else:
            assert not out or not h.value       # no handle behind a refusal
        return rc, err, (_launches(fb, p) if timed else 0)

    def refused(p, cause, **kw):
        rc, err, nl = call(p, **kw)
        assert rc != 0 and b"fb_lss_dconnect" in err and cause in err and nl == 0, (cause, err, nl)

    refused(None, b"null handle", timed=False)
    r = fb.Robot2DWorld(n)
    refused(r._h, b"the plant is not a LinearizedSS handle", timed=False)      # (a Robot2D handle keeps no per-launch stamps)
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.dconnect(r, feedback=np.zeros((1, 1)), inputs=np.ones((1, 1)), reads=[0])
    w = mk(3, 2, 4)
    refused(w._h, b"the compensator is not a LinearizedSS handle", c=r._h)
    r.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 3, n, 0, C.byref(h)) == 0
    refused(h, b"the plant has no model yet")
    refused(w._h, b"the compensator has no model yet", c=h)
    fb.lib.fb_destroy(h)
    # a continuous operand: the d verbs' wording; fb_lss_connect keeps its own for a sampled one
    cont = fb.LinearWorld(lss(2, 1, 1))
    refused(cont._h, b"a discrete-time verb on a continuous model")
    refused(w._h, b"a discrete-time verb on a continuous model", c=cont._h)
    one, g = np.zeros(1, dtype=np.int32), np.ones(8)
    hh = C.c_void_p(1)
    assert fb.lib.fb_timing_begin_per_launch(w._h, 8) == 0
    rc = fb.lib.fb_lss_connect(w._h, None, pi32(one), 1, pd(g), 0, pd(g), 0, 1, pi32(one), 1, None, C.byref(hh))
    err = fb.lib.fb_last_error()
    assert rc != 0 and b"fb_lss_connect: a continuous-time verb on a sampled model" in err and not hh.value and _launches(fb, w._h) == 0
    rc = fb.lib.fb_lss_connect(cont._h, w._h, pi32(one), 1, pd(g), 0, pd(g), 0, 1, pi32(one), 1, None, C.byref(hh))
    assert rc != 0 and b"fb_lss_connect: a continuous-time verb on a sampled model" in fb.lib.fb_last_error() and not hh.value
    cont.close()
    # another Ts, in the last bit: both values are printed with 17 digits
    ts2 = float(np.nextafter(TS, 1.0))
    off = mk(2, 1, 1, Ts=ts2)
    refused(w._h, ("Ts = %.17g differs from the plant's Ts = %.17g" % (ts2, TS)).encode(), c=off._h)
    off.close()
    other = mk(2, 1, 1, nn=n + 1)
    refused(w._h, b"the compensator has N = 6 systems, the plant N = 5", c=other._h)
    other.close()
    big, big2 = mk(20, 8, 64), mk(12, 8, 64)
    refused(big._h, b"nx_p + nx_c + nd = 33", c=big2._h, dz=(0,))
    rc, err, nl = call(big._h, c=big2._h)                     # nx' = 32, nv = 16, nz = 128: a successful call stamps the kernel once
    assert rc == 0 and nl == 1, err
    big3 = mk(11, 8, 64, seed=4)
    refused(big._h, b"nz + nd = ny_p + ny_c + nd = 129", c=big3._h, dz=(0,))
    refused(w._h, b"nd = -1", nd=-1)
    refused(w._h, b"nd = 32", dz=(0,) * 32)
    refused(w._h, b"nd = 2 and dz is NULL", dz=None, nd=2)
    refused(w._h, b"dz[1] = 4 is outside [0, 4)", dz=(0, 4))
    refused(w._h, b"dz[0] = -1 is outside", dz=(-1,))
    refused(w._h, b"nf = 0", jz=(), nf=0)
    refused(w._h, b"nf = 33", jz=(0,) * 33)
    refused(w._h, b"nw = 0", nw=0)
    refused(w._h, b"nw = 9", nw=9)
    refused(w._h, b"ny = 0", iz=(), ny=0)
    refused(w._h, b"ny = 65", iz=(0,) * 65)
    refused(w._h, b"jz[1] = 4 is outside [0, 4)", jz=(0, 4))
    refused(w._h, b"jz[1] = 6 is outside [0, 6)", jz=(5, 6), dz=(1, 1))
    refused(w._h, b"jz[0] = -1 is outside", jz=(-1,))
    refused(w._h, b"iz[0] = 5 is outside [0, 5)", iz=(5,), dz=(3,))
    refused(w._h, b"F, G and jz are required", F=False)
    refused(w._h, b"F, G and jz are required", G=False)
    refused(w._h, b"F, G and jz are required", jz=None, nf=1)
    refused(w._h, b"out is null", out=False)
    c9 = mk(2, 8, 64, seed=1)
    refused(big._h, b"iz is NULL", c=c9._h, iz=None)
    w60 = mk(3, 2, 60, seed=6)
    refused(w60._h, b"iz is NULL (every row of [z; q]) and nz + nd = 65", iz=None, dz=(0,) * 5)
    rc, err, nl = call(w._h, iz=None, dz=(1, 1), jz=(5, 0))          # every row of [z; q]; a row delayed twice over; a read now and one late
    assert rc == 0 and nl == 1, err
    with pytest.raises(KeyError, match="not a signal label"):
        fb.dconnect(w, feedback=np.zeros((2, 1)), inputs=np.ones((2, 1)), reads=["nope"])
    with pytest.raises(KeyError, match="not a signal label"):
        fb.dconnect(w, feedback=np.zeros((2, 1)), inputs=np.ones((2, 1)), reads=["yp0[k-1]"])          # (not delayed in this call)
    with pytest.raises(ValueError, match="feedback must be"):
        fb.dconnect(w, feedback=np.zeros((3, 1)), inputs=np.ones((2, 1)), reads=[0])
    for x in (w, big, big2, big3, c9, w60):
        x.close()
