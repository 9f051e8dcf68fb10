"""fb_lss_stepinfo (flightbatch.timeresp): step responses and StepInfo of a batch of LinearizedSS models on the device, pinned by

  1. exact discretisation on random stable plants of every group size, through the numpy restatement of the kernel
     (tests/timeresp_prototype.py; tests/test_timeresp_host.py holds the prototype itself to the exact side first), with caller-given
     endpoints and thresholds;
  2. batch shapes: a lone group, a partial wave, a tail block, bit for bit;
  3. strides, and the info without a sample buffer;
  4. repeatability and position independence, bit for bit, and the handle left as it was;
  5. the Model(lss) stepper driven with the same step input;
  6. diverging, flat and never-rising pairs, flagged in place among healthy neighbours;
  7. the two StepInfo tables the reference's robot2d design notebook stores, from linearize on the device to show;
  8. the refusals of the C ABI on a live device;
  9. examples/loop_responses.py.

The shared bound (the family's rule): the device differs from the prototype in FMA contraction and <= 1-ulp division only, so it may deviate from
the exact side ten times as far as the prototype does over the same pairs, with a floor of 1e-11, every deviation scaled by max|y| of its
pair. Peak, settling and rise time are index times dt and are compared for equality on every pair: tests/test_timeresp_host.py shows that on
these pairs every deciding sample sits at least 1e-9 of the step size from its threshold."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import timeresp_prototype as proto
from support import clock

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR, MARGIN = 1e-11, 10.0
N_STEPS = int(round(proto.T_SIM / proto.DT))
VALUES, PERCENT, TIMES = (0, 1, 2, 3), (5, 6), (4, 7, 8)      # rows of info


@functools.lru_cache(maxsize=None)
def _reference(nx, n=proto.N_SYS):
    """plants, pairs, RK4 and exact samples of one size (computed once, read only)"""
    sysm = proto.plants(nx, n)
    P = proto.pairs(*sysm, proto.CHANNELS)
    Y, Ye = proto.samples_rk4(*P, N_STEPS, proto.DT), proto.samples_exact(*P, N_STEPS, proto.DT)
    for a in (*sysm, *P, Y, Ye):
        a.setflags(write=False)
    return sysm, P, Y, Ye


def _world(fb, sysm, sel=slice(None), x0=None):
    return fb.LinearWorld(proto.model(fb, *[np.ascontiguousarray(a[sel]) for a in sysm], x0=x0))


def _raw(fb, w, channels, t_sim=proto.T_SIM, dt=proto.DT, opts=None, y0=None, yf=None, stride=1, want_y=True):
    """the C ABI itself: (y [ns, m, n] or None, info [9, m, n], status [m, n])"""
    iu = np.array([c[0] for c in channels], dtype=np.int32); iy = np.array([c[1] for c in channels], dtype=np.int32)
    m, n = len(channels), w.n
    N = int(round(t_sim / dt))
    y = np.full((fb.timeresp.samples(N, stride), m, n), np.nan) if want_y else None
    info, status = np.full((9, m, n), np.nan), np.full((m, n), -1, dtype=np.int32)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    o = None if opts is None else np.array(opts, dtype=np.float64)
    y0 = None if y0 is None else np.ascontiguousarray(y0, dtype=np.float64)
    yf = None if yf is None else np.ascontiguousarray(yf, dtype=np.float64)
    rc = fb.lib.fb_lss_stepinfo(w._h, pi(iu), pi(iy), m, t_sim, dt, pd(o), pd(y0), pd(yf), stride, pd(y), pd(info), pi(status))
    assert rc == 0, fb.lib.fb_last_error()
    return y, info, status


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _info_dev(info, info_e, Ye):
    """worst deviation of the value rows and of the two percentages from the exact side's, scaled by max|y| of the pair (a percentage:
    by 100 max|y| / stepsize (1 + |value| / 100), what an error of max|y| in peak, yf, y0 and stepsize moves it by)"""
    ymax = np.abs(Ye).max(axis=0)
    dv = max(float((np.abs(info[k] - info_e[k]) / ymax).max()) for k in VALUES)
    dp = max(float((np.abs(info[k] - info_e[k]) / (100.0 * ymax / info_e[2] * (1.0 + np.abs(info_e[k]) / 100.0))).max()) for k in PERCENT)
    return dv, dp


# ---- 1. every size against the exact side, with the endpoints and thresholds a caller may give -------------------------------------------------
@pytest.mark.parametrize("nx", proto.NX_ALL)
def test_samples_and_info_against_the_exact_side(fb, nx, capsys):
    sysm, P, Y, Ye = _reference(nx)
    n, m = proto.N_SYS, len(proto.CHANNELS)
    w = _world(fb, sysm)
    res = fb.timeresp.step(w, proto.CHANNELS, proto.T_SIM, dt=proto.DT)
    assert res.y.shape == (n, m, N_STEPS + 1) and res.t.shape == (N_STEPS + 1,) and res.t[-1] == N_STEPS * proto.DT and (res.status == 0).all()
    Yd = res.y.transpose(2, 1, 0).reshape(N_STEPS + 1, m * n)
    d, p = proto.sample_dev(Yd, Ye), proto.sample_dev(Y, Ye)
    with capsys.disabled():
        print(f"\n[fb_lss_stepinfo vs exact] nx {nx:2d}, {n} x {m}, N {N_STEPS}: samples {d.max():.2e} of max|y| (prototype {p.max():.2e}; device vs "
              f"prototype {proto.sample_dev(Yd, Y).max():.2e})", end="")
    assert d.max() <= max(MARGIN * p.max(), FLOOR)
    assert _same(res.y[:, 1], res.y[:, 3])           # (the channel asked for twice)
    for name, (y0_in, yf_in, opts) in proto.gpu_variants(P, Y).items():
        shape = lambda a: None if a is None else a.reshape(m, n).T
        si = fb.stepinfo(w, proto.CHANNELS, proto.T_SIM, dt=proto.DT, y0=shape(y0_in), yf=shape(yf_in), settling_th=opts[0], risetime_th=opts[1:])
        info = np.array([getattr(si, f).T.reshape(-1) for f in proto.FIELDS])
        info_p, st_p = proto.stepinfo_batch(Y, proto.DT, y0_in, yf_in, opts)
        info_e, st_e = proto.stepinfo_batch(Ye, proto.DT, y0_in, yf_in, opts)
        (dv, dp), (pv, pp) = _info_dev(info, info_e, Ye), _info_dev(info_p, info_e, Ye)
        with capsys.disabled():
            print(f"\n    {name:10s}: values {dv:.2e} (prototype {pv:.2e}), percentages {dp:.2e} ({pp:.2e}); NaN rise times {int(np.isnan(info[8]).sum())}; "
                  f"indices differing from the prototype's {int((~np.isclose(info[list(TIMES)], info_p[list(TIMES)], rtol=0, atol=0, equal_nan=True)).sum())}", end="")
        assert (si.status == 0).all() and si.ok.all() and (st_p == 0).all() and (st_e == 0).all()
        assert dv <= max(MARGIN * pv, FLOOR) and dp <= max(MARGIN * pp, FLOOR), name
        for k in TIMES:
            assert np.array_equal(info[k], info_p[k], equal_nan=True), (name, proto.FIELDS[k])
    w.close()


# ---- 2. batch shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [7, 8, 31])
def test_batch_shapes_give_the_same_bits(fb, nx):
    sysm = proto.plants(nx, 130)
    runs = {}
    for n, m in ((9, 4), (130, 1), (1, 1), (1, 4), (3, 1), (3, 4), (9, 1), (63, 1)):
        w = _world(fb, sysm, slice(0, n))
        runs[n, m] = _raw(fb, w, proto.CHANNELS[:m])
        w.close()
        assert (runs[n, m][2] == 0).all()
    for (n, m), (y, info, status) in runs.items():
        for big in ((9, 4), (130, 1)):
            if (n, m) != big and n <= big[0] and m <= big[1]:
                yb, ib, sb = runs[big]
                assert _same(y, yb[:, :m, :n]) and _same(info, ib[:, :m, :n]) and np.array_equal(status, sb[:m, :n]), ((n, m), big)


# ---- 3. strides ----------------------------------------------------------------------------------------------------------------------------------
def test_strides_and_no_sample_buffer(fb):
    sysm = _reference(8)[0]
    w = _world(fb, sysm)
    y1, info1, st1 = _raw(fb, w, proto.CHANNELS)
    assert y1.shape[0] == N_STEPS + 1 and not np.isnan(y1).any()
    for stride in (7, N_STEPS, N_STEPS + 5):
        y, info, st = _raw(fb, w, proto.CHANNELS, stride=stride)
        rows = list(range(0, N_STEPS, stride)) + [N_STEPS]
        assert y.shape[0] == len(rows) == -(-N_STEPS // stride) + 1
        assert _same(y, y1[rows]) and _same(info, info1) and np.array_equal(st, st1), stride
        res = fb.timeresp.step(w, proto.CHANNELS, proto.T_SIM, dt=proto.DT, stride=stride)
        assert np.array_equal(res.t, np.array(rows) * proto.DT) and _same(res.y.transpose(2, 1, 0), y)
    _, info, st = _raw(fb, w, proto.CHANNELS, want_y=False)
    assert _same(info, info1) and np.array_equal(st, st1)
    w.close()


# ---- 4. repeatability, position independence, and nothing written on the handle -----------------------------------------------------------------
def test_bitwise_repeatable_and_the_handle_untouched(fb):
    sysm = _reference(12)[0]
    rng = np.random.default_rng(4)
    w = _world(fb, sysm, x0=rng.standard_normal((proto.N_SYS, 12)))
    w.u = rng.standard_normal((proto.NU, proto.N_SYS))
    w.step(7, dt=1e-3)
    w.sync()
    snap = lambda: (w.x, w.u, *clock(fb, w), w.status, *w.model())
    before = snap()
    first = _raw(fb, w, proto.CHANNELS)
    again = _raw(fb, w, proto.CHANNELS)
    after = snap()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[2] == pytest.approx(7e-3) and before[3] == 7
    assert (first[2] == 0).all()
    same = lambda a, b: _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2])
    pick = lambda r, ch, sel: (r[0][:, ch][:, :, sel], r[1][:, ch][:, :, sel], r[2][ch][:, sel])
    allc, alls = list(range(4)), list(range(proto.N_SYS))
    assert same(first, again)
    w.close()
    w = _world(fb, sysm, slice(None, None, -1))
    assert same(pick(first, allc, alls[::-1]), _raw(fb, w, proto.CHANNELS))
    w.close()
    sub = [8, 0, 5, 3]
    w = _world(fb, sysm, sub)
    assert same(pick(first, allc, sub), _raw(fb, w, proto.CHANNELS))
    w.close()
    w = _world(fb, sysm)
    perm = [2, 0, 3, 1]
    assert same(pick(first, perm, alls), _raw(fb, w, [proto.CHANNELS[k] for k in perm]))
    assert same(pick(first, [2], alls), _raw(fb, w, [proto.CHANNELS[2]]))
    w.close()


# ---- 5. the stepper with the same input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [7, 16, 31])
def test_cross_check_with_the_lss_stepper(fb, nx, capsys):
    sysm = _reference(nx)[0]
    w = _world(fb, sysm)
    y, _, st = _raw(fb, w, proto.CHANNELS)
    assert (st == 0).all()
    worst = 0.0
    for iu in range(proto.NU):
        u = np.zeros((proto.NU, proto.N_SYS)); u[iu] = 1.0
        w.set_state(np.zeros((nx, proto.N_SYS)))
        w.u = u
        w.set_params(dt=proto.DT)
        for k in range(0, N_STEPS + 1, 100):
            w.f_ode()
            ys = w.y
            for j, (cu, cy) in enumerate(proto.CHANNELS):
                if cu == iu:
                    worst = max(worst, float((np.abs(ys[cy] - y[k, j]) / np.maximum(np.abs(y[k, j]), 1.0)).max()))
            if k < N_STEPS:
                w.step(100)
        w.sync()
    w.close()
    with capsys.disabled():
        print(f"\n[fb_lss_stepinfo vs fb_step + fb_f_ode] nx {nx:2d}: {worst:.2e} of max(|y|, 1) over 21 samples x {proto.N_SYS} x 4", end="")
    assert worst <= 1e-11


# ---- 6. failure pairs in place --------------------------------------------------------------------------------------------------------------------
def test_failure_pairs_are_flagged_in_place(fb):
    sysm, ch, yf = proto.failure_case()
    w = _world(fb, sysm)
    y, info, st = _raw(fb, w, ch, yf=yf)
    w.close()
    P = proto.pairs(*sysm, ch)
    info_p, st_p = proto.stepinfo_batch(proto.samples_rk4(*P, N_STEPS, proto.DT), proto.DT, None, yf.reshape(-1))
    want = np.zeros((3, 7), dtype=np.int32)
    want[:, 2] = proto.DIVERGED
    want[1, 4] = proto.FLAT
    assert np.array_equal(st, want) and np.array_equal(st_p.reshape(3, 7), want)
    assert np.isnan(info[:, :, 2]).all() and not (np.abs(y[:, :, 2]) <= proto.BLOWUP).all(axis=0).any()
    assert np.array_equal(info[:5, 1, 4], np.zeros(5)) and np.isnan(info[5:, 1, 4]).all() and (y[:, 1, 4] == 0.0).all()
    assert st[0, 5] == 0 and np.isnan(info[8, 0, 5]) and info[1, 0, 5] == 100.0 and info[7, 0, 5] == N_STEPS * proto.DT
    assert np.array_equal(np.isnan(info), np.isnan(info_p.reshape(9, 3, 7)))
    for k in (4, 7, 8):
        assert np.array_equal(info[k], info_p[k].reshape(3, 7), equal_nan=True)
    keep = [0, 1, 3, 6]
    w = _world(fb, sysm, keep)
    yh, ih, sh = _raw(fb, w, ch)
    w.close()
    assert (sh == 0).all() and _same(yh, y[:, :, keep]) and _same(ih, info[:, :, keep])


# ---- 7. the notebook's tables, end to end -----------------------------------------------------------------------------------------------------------
def test_the_notebooks_tables_from_linearize_to_show(fb, capsys):
    w = fb.Robot2DWorld(3)
    lss = fb.linearize(w, None, scheme="forward")
    lw = fb.linear_world(w)
    w.close()
    A, B = lw.model()
    open_loop = fb.stepinfo(lw, [(0, 0)], 0.5, dt=0.005)
    lw.close()
    assert np.array_equal(A[0], lss.A[0]) and np.array_equal(B[0], lss.B[0])
    for f in proto.FIELDS:
        v = getattr(open_loop, f)
        assert v.shape == (3, 1) and np.array_equal(v, np.broadcast_to(v[:1], v.shape), equal_nan=True)
    tables = proto.stored_tables()
    loops = dict(zip(("velocity_loop", "position_loop"), proto.notebook_loops(A[0], B[0])))
    labels = {"velocity_loop": ("v_ref", "v"), "position_loop": ("η_ref", "η")}
    stable = {}
    for which, (Al, b, c, d) in loops.items():
        t = tables[which]
        cw = fb.LinearWorld(proto.loop_model(fb, Al, b, c, d, labels=labels[which]))
        si = fb.stepinfo(cw, [labels[which]], t["t_sim"], dt=t["dt"])
        stable[which] = bool(fb.poles(cw).stable[0])
        cw.close()
        text = si.show(0, 0)
        with capsys.disabled():
            print(f"\n[fb_lss_stepinfo, Robot2D {which}] " + "; ".join(" ".join(s.split()) for s in text.split("\n")), end="")
        assert si.ok.all()
        proto.assert_matches_table(text.split("\n"), which)
        if which == "position_loop":
            N = int(round(t["t_sim"] / t["dt"]))
            assert si.peaktime[0, 0] == N * t["dt"] and abs(si.peaktime[0, 0] - 9.995) <= 0.005 + 1e-12
    assert stable == {"velocity_loop": False, "position_loop": True}      # (η integrates v: the velocity loop keeps the pole at zero)


# ---- 8. refusals on a live device ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 5
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def call(h, nsys=n, iu=(0,), iy=(0,), m=None, t_sim=1.0, dt=0.01, opts=None, stride=1, info=True, status=True):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        m = len(iu) if m is None else m
        cu, cy = np.array(iu, dtype=np.int32), np.array(iy, dtype=np.int32)
        mm = max(min(m, 64), 1)
        out, st = np.empty((9, mm, nsys if nsys <= 1000 else 1)), np.empty((mm, nsys if nsys <= 1000 else 1), dtype=np.int32)
        o = None if opts is None else np.array(opts, dtype=np.float64)
        rc = fb.lib.fb_lss_stepinfo(h, pi(cu), pi(cy), m, t_sim, dt, pd(o), None, None, stride, None, pd(out) if info else None, pi(st) if status else None)
        return rc, fb.lib.fb_last_error(), launches(h)

    def refused(h, cause, **kw):
        rc, err, nl = call(h, **kw)
        assert rc != 0 and b"fb_lss_stepinfo" in err and cause in err and nl == 0, (cause, err, nl)

    info, st = np.empty(9), np.empty(1, dtype=np.int32)
    ch = np.zeros(1, dtype=np.int32)
    assert fb.lib.fb_lss_stepinfo(None, pi(ch), pi(ch), 1, 1.0, 0.01, None, None, None, 1, None, pd(info), pi(st)) != 0
    assert b"null handle" in fb.lib.fb_last_error()
    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(ac._h, b"not a LinearizedSS handle")
    ac.close()
    r = fb.Robot2DWorld(n)
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.stepinfo(r, [(0, 0)], 1.0, dt=0.01)
    r.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 3, n, 0, C.byref(h)) == 0
    refused(h, b"no model yet")
    fb.lib.fb_destroy(h)
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(32, 1, 1, n, 0, C.byref(h)) == 0
    refused(h, b"FB_STEPINFO_NX_MAX")
    fb.lib.fb_destroy(h)
    big = (2 ** 31) // 64
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(1, 1, 1, big, 0, C.byref(h)) == 0, fb.lib.fb_last_error()
    refused(h, b"2^31 - 1 pairs", nsys=big, iu=(0,) * 64, iy=(0,) * 64)
    fb.lib.fb_destroy(h)

    w = _world(fb, proto.plants(3, n))
    refused(w._h, b"1 <= m <= 64", m=0)
    refused(w._h, b"1 <= m <= 64", iu=(0,) * 65, iy=(0,) * 65)
    refused(w._h, b"iu[1] = 2 is outside", iu=(0, proto.NU), iy=(0, 0))
    refused(w._h, b"iy[0] = -1 is outside", iy=(-1,))
    refused(w._h, b"iy[0] = 3 is outside", iy=(proto.NY,))
    for dt in (0.0, -0.01, np.inf, np.nan):
        refused(w._h, b"must be positive and finite", dt=dt)
    refused(w._h, b"at least dt", t_sim=0.005)
    refused(w._h, b"at least dt", t_sim=np.inf)
    refused(w._h, b"at most 200000", t_sim=2001.0)
    refused(w._h, b"stride = 0", stride=0)
    for opts in ((0.02, 0.9, 0.1), (0.02, 0.0, 0.9), (0.02, 0.1, 1.0), (0.02, 0.5, 0.5), (0.02, np.nan, 0.9)):
        refused(w._h, b"0 < lo < hi < 1", opts=opts)
    for opts in ((0.0, 0.1, 0.9), (-0.02, 0.1, 0.9), (np.nan, 0.1, 0.9)):
        refused(w._h, b"settling_th", opts=opts)
    refused(w._h, b"info and status are required", info=False)
    refused(w._h, b"info and status are required", status=False)
    rc, err, nl = call(w._h)
    assert rc == 0 and nl == 1, err
    rc, err, nl = call(w._h, t_sim=2000.0)       # 200000 steps: the limit itself
    assert rc == 0 and nl == 1, err
    with pytest.raises(KeyError, match="not an output label"):
        fb.stepinfo(w, [("u0", "nope")], 1.0, dt=0.01)
    assert fb.timeresp.default_dt(w) == float("%.1e" % (1.0 / (12.0 * fb.poles(w).wn.max())))
    w.close()


# ---- 9. the example ------------------------------------------------------------------------------------------------------------------------------------
def test_the_loop_responses_example_prints_the_two_tables():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "loop_responses.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for which in ("velocity_loop", "position_loop"):
        for k, line in enumerate(proto.stored_tables()[which]["lines"]):
            if not (which == "position_loop" and k == 4):
                assert line in out.stdout, line
    assert "q <- q_ref" in out.stdout and out.stdout.count("\n") >= 28 + 9
