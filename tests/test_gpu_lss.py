"""Model(lss) on the device (FB_MODEL_LSS: csrc/lss_kernels.hpp, csrc/fb_lss.inc, flightbatch.lss) against numpy on the host.

The host reference is numpy fp64 with an explicit column loop (and, for trajectories, the same RK4 in np.longdouble); it shares no code
with the kernels. Bounds:
  f_ode      each component within the dot-product bound (nx + nu + 2) 2^-53 (|c| + sum |a_rc dx_c| + sum |b_rc du_c|), which covers any
             summation order and any FMA contraction of the nx + nu products and their additions;
  1000 steps 1e-11 scaled by max(|x|, 1) per row against the longdouble RK4 (the figure the README holds the C172 stepper to), after the
             precondition that numpy fp64 stays within 1e-13 of it. Measured worst device value: docs/design/linearize.md."""
import ctypes as C

import numpy as np
import pytest

from support import LSS_N_TRAJ as N_TRAJ, LSS_NSTEPS as NSTEPS, affine, exchange, lss_run_device as run_device, make_lss, pd as _pd, traj_case

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def check_f_ode(fb, m, x, u):
    """x [n, nx], u [n, nu]: the device's xdot and y at (x, u) against the column loop, component by component"""
    n, nx = x.shape
    nu, ny = u.shape[1], m.y0.shape[1]
    w = fb.LinearWorld(m)
    assert (w.nx, w.nu, w.ny, w.n, w.ns) == (nx, nu, ny, n, 0)
    assert np.array_equal(w.x, m.x0.T) and np.array_equal(w.u, m.u0.T)      # Modeling.X(lss) = copy(x0), U = copy(u0)
    w.x = x.T
    w.u = u.T
    xd = np.empty((nx, n))
    w.f_ode(xd)
    y = w.y
    dx, du = x - m.x0, u - m.u0
    xd_ref, xd_mag = affine(m.xdot0, m.A, dx, m.B, du)
    y_ref, y_mag = affine(m.y0, m.C, dx, m.D, du)
    k = (nx + nu + 2) * U
    ex, ey = np.abs(xd.T - xd_ref) / (k * xd_mag), np.abs(y.T - y_ref) / (k * y_mag)
    print(f"\n[lss f_ode {nx}/{nu}/{ny} n={n}] worst error / bound: xdot {ex.max():.3f}, y {ey.max():.3f}", end="")
    assert (ex <= 1.0).all() and (ey <= 1.0).all()
    w.close()


# ---- 1. the reference's own known-answer test (FP test_linearization.jl:14-57) ---------------------------------------------------------
def test_reference_known_answer(fb, capsys):
    x0, u0, y0 = np.array([1, 0.5, 0.3, 5.0]), np.array([0.1, 0.2]), np.array([0.3, 0.8, 2, 3, -9.8])
    m = fb.LinearizedSS(xdot0=x0[None], x0=x0[None], u0=u0[None], y0=y0[None], A=np.outer(x0, x0)[None], B=np.outer(x0, u0)[None],
                        C=np.outer(y0, x0)[None], D=np.outer(y0, u0)[None], x_labels=tuple("abcd"), u_labels=tuple("pq"), y_labels=tuple("vwxyz"))
    with capsys.disabled():
        check_f_ode(fb, m, 2 * x0[None], 3 * u0[None])
    # and the numbers themselves: xdot = x0 (1 + x0.x0 + 2 u0.u0), y = y0 (1 + x0.x0 + 2 u0.u0)
    w = fb.LinearWorld(m)
    w.x, w.u = 2 * x0[:, None], 3 * u0[:, None]
    xd = np.empty((4, 1))
    w.f_ode(xd)
    g = 1 + x0 @ x0 + 2 * (u0 @ u0)
    assert np.allclose(xd[:, 0], x0 * g, rtol=1e-14, atol=0) and np.allclose(w.y[:, 0], y0 * g, rtol=1e-14, atol=0)
    w.close()


# ---- 2. shapes and edges ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (4, 1, 6), (5, 2, 3), (8, 2, 3), (9, 3, 17), (16, 4, 33), (17, 4, 5), (20, 4, 38), (32, 8, 64)]


@pytest.mark.parametrize("n", [1, 63, 130])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_f_ode_shapes_and_batch_edges(fb, shape, n, capsys):
    nx, nu, ny = shape
    m = make_lss(fb, nx, nu, ny, n, seed=1000 * nx + n)
    rng = np.random.default_rng(7 * nx + n)
    with capsys.disabled():
        check_f_ode(fb, m, m.x0 + rng.standard_normal((n, nx)), m.u0 + rng.standard_normal((n, nu)))


# ---- 3. trajectories -------------------------------------------------------------------------------------------------------------------
TRAJ_SHAPES = [(4, 1, 6), (16, 4, 33), (20, 4, 38)]
@pytest.mark.parametrize("shape", TRAJ_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_trajectory_against_longdouble_rk4(fb, shape, capsys):
    case = traj_case(fb, shape)
    x_ld, x_64 = case[4], case[5]
    scale = np.maximum(np.abs(x_ld), 1.0).astype(np.float64)
    pre = float((np.abs(x_64 - x_ld).astype(np.float64) / scale).max())
    assert pre <= 1e-13, f"precondition: numpy fp64 is {pre:.3e} from the longdouble RK4 (change the inputs, not the number)"
    x = run_device(fb, case, 50)
    err = float((np.abs(x - x_ld).astype(np.float64) / scale).max())
    with capsys.disabled():
        print(f"\n[lss rk4 {shape} n={N_TRAJ}, {NSTEPS} steps] scaled error vs longdouble: numpy fp64 {pre:.3e}, device {err:.3e}", end="")
    assert err <= 1e-11


# ---- 4. launch partition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TRAJ_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_launch_partition_gives_the_same_bits(fb, shape):
    case = traj_case(fb, shape)
    ref = run_device(fb, case, 50)
    for spl in (1, 7):
        assert np.array_equal(run_device(fb, case, spl), ref), spl
    assert np.array_equal(run_device(fb, case, 50, cuts=([1, 36, 63], [450, 13, 437])), ref)
    assert np.array_equal(run_device(fb, case, 7, cuts=([99, 1], [3] * 300)), ref)


# ---- 5. device-to-device construction --------------------------------------------------------------------------------------------------
def _same_bits_after_run(fb, wa, wb, rng):
    assert (wa.nx, wa.nu, wa.ny, wa.n) == (wb.nx, wb.nu, wb.ny, wb.n)
    assert wa.x_labels == wb.x_labels and wa.u_labels == wb.u_labels and wa.y_labels == wb.y_labels
    xa, xb = np.empty((wa.nx, wa.n)), np.empty((wa.nx, wa.n))
    wa.f_ode(xa); wb.f_ode(xb)                                        # at (x0, u0): xdot0 and y0 themselves
    assert np.array_equal(xa, xb) and np.array_equal(wa.y, wb.y) and np.array_equal(wa.x, wb.x) and np.array_equal(wa.u, wb.u)
    dx, du = 1e-2 * rng.standard_normal((wa.nx, wa.n)), 1e-2 * rng.standard_normal((wa.nu, wa.n))
    for w in (wa, wb):
        w.x = w.x + dx
        w.u = w.u + du
    wa.f_ode(xa); wb.f_ode(xb)                                        # off the point: every column of A, B, C, D takes part
    assert np.array_equal(xa, xb) and np.array_equal(wa.y, wb.y)
    for w in (wa, wb):
        w.step(100, dt=0.01, steps_per_launch=50)
        w.f_ode()
    assert np.array_equal(wa.x, wb.x) and np.array_equal(wa.y, wb.y) and np.isfinite(wa.x).all()
    return xa


def test_device_to_device_construction(fb):
    n = 8
    w = fb.BatchedWorld(n, kinematics="NED")
    tp = fb.TrimParameters(EAS=np.linspace(35.0, 55.0, n), h_e=np.linspace(300.0, 2500.0, n), flaps=np.array([0, 0, 0.5, 1.0, 0, 0.25, 0, 0]))
    lss = fb.linearize(w, tp)
    assert lss.success.all() and (lss.status == 0).all()
    rng = np.random.default_rng(3)
    # every index
    wd, wh = fb.linear_world(w), fb.LinearWorld(lss)
    assert (wd.nx, wd.nu, wd.ny) == (16, 4, 33) and wd.x_labels == lss.x_labels
    assert np.array_equal(wd.x, lss.x0.T) and np.array_equal(wd.u, lss.u0.T)
    xd = _same_bits_after_run(fb, wd, wh, rng)
    assert np.abs(xd).max() > 0
    wd.close(); wh.close()
    # a longitudinal selection against subsystem() on the host
    sel = dict(x=("q", "θ", "v_x", "v_z"), u=("elevator",), y=("q", "θ", "α"))
    sub = fb.subsystem(lss, **sel)
    wd, wh = fb.linear_world(w, **sel), fb.LinearWorld(sub)
    assert (wd.nx, wd.nu, wd.ny) == (4, 1, 3) and wd.x_labels == sel["x"] and wd.y_labels == sel["y"]
    _same_bits_after_run(fb, wd, wh, rng)
    wd.close(); wh.close()
    # an index outside the source's vectors is refused, not followed
    bad = np.array([0, 16], dtype=np.int32)
    h = C.c_void_p()
    assert fb.lib.fb_lss_from_linearization(w._h, bad.ctypes.data_as(C.POINTER(C.c_int32)), 2, None, 0, None, 0, C.byref(h)) != 0
    assert b"outside" in fb.lib.fb_last_error() and not h.value
    # the last linearisation did not write A | B: refused with a message
    nx, nu, ny = 16, 4, 33
    b = [np.empty((k, n)) for k in (nx, nx, nu, ny)] + [np.empty(ny * nx * n), np.empty(ny * nu * n)]
    st = np.zeros(n, dtype=np.int32)
    assert fb.lib.fb_linearize_state(w._h, fb.K["FB_LIN_FORWARD"], _pd(b[0]), _pd(b[1]), _pd(b[2]), _pd(b[3]), None, None, _pd(b[4]), _pd(b[5]),
                                     st.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    with pytest.raises(fb.FlightBatchError, match=r"did not write A \| B"):
        fb.linear_world(w)
    w.close()
    # no linearisation has run
    r = fb.Robot2DWorld(4)
    with pytest.raises(fb.FlightBatchError, match="no linearisation has run"):
        fb.linear_world(r)
    r.close()


# every source model, both exchanges (k_lss_gather's index arithmetic with snx = 20 and snx = 4; fb_lss_from_linearization reads
# FLIGHTBATCH_LSS_EXCHANGE as fb_lss_create does). Selections are given in an order that is not ascending.
def _linearized_x2(fb):
    n = 8
    w = fb.Cessna172Xv2World(n, kinematics="NED")
    tp = fb.TrimParameters(EAS=np.linspace(35.0, 55.0, n), h_e=np.linspace(300.0, 2500.0, n), flaps=np.array([0, 0, 0.5, 1.0, 0, 0.25, 0, 0]))
    lss = fb.linearize(w, tp)
    assert lss.success.all() and (lss.status == 0).all()
    sel = dict(x=("r", "φ", "v_y", "p", "β_filt", "rud_p", "ail_p"), u=("rudder_cmd", "aileron_cmd"), y=("β", "p", "χ", "φ", "r", "ail_p"))
    return w, lss, (20, 4, 38), sel, (7, 2, 6)


def _linearized_robot2d(fb):
    n = 8
    rng = np.random.default_rng(29)
    w = fb.Robot2DWorld(n)
    lss = fb.linearize(w, fb.InitParameters(u_m=rng.uniform(-0.2, 0.2, n), ω=rng.uniform(-0.05, 0.05, n), η=rng.uniform(-1, 1, n)))
    assert (lss.status == 0).all() and np.abs(lss.A[1:] - lss.A[:-1]).max() > 0
    return w, lss, (4, 1, 6), dict(x=("θ", "ω"), u=("m",), y=("τ_m", "θ")), (2, 1, 2)


@pytest.mark.parametrize("name", ["panel", "shfl"])
@pytest.mark.parametrize("source", [_linearized_x2, _linearized_robot2d], ids=["c172x2", "robot2d"])
def test_device_to_device_construction_from_every_source(fb, source, name):
    w, lss, full, sel, part = source(fb)
    rng = np.random.default_rng(5)
    with exchange(name):
        wd, wh = fb.linear_world(w), fb.LinearWorld(lss)
        assert wd.exchange == name and wh.exchange == name
        assert (wd.nx, wd.nu, wd.ny) == full and wd.x_labels == lss.x_labels and wd.y_labels == lss.y_labels
        assert np.array_equal(wd.x, lss.x0.T) and np.array_equal(wd.u, lss.u0.T)
        xd = _same_bits_after_run(fb, wd, wh, rng)
        assert np.abs(xd).max() > 0
        wd.close(); wh.close()
        sub = fb.subsystem(lss, **sel)
        wd, wh = fb.linear_world(w, **sel), fb.LinearWorld(sub)
        assert wd.exchange == name and wh.exchange == name
        assert (wd.nx, wd.nu, wd.ny) == part and wd.x_labels == sel["x"] and wd.u_labels == sel["u"] and wd.y_labels == sel["y"]
        assert np.array_equal(wd.x, sub.x0.T) and np.array_equal(wd.u, sub.u0.T)
        A, B = wd.model()                      # the handle's own copy: the selected rows and columns, in the order given
        assert np.array_equal(A, sub.A) and np.array_equal(B, sub.B)
        _same_bits_after_run(fb, wd, wh, rng)
        wd.close(); wh.close()
    w.close()


@pytest.mark.parametrize("missing", ["x0", "u0", "A | B", "C | D"])
def test_a_block_the_last_linearisation_did_not_write_is_refused_by_name(fb, missing):
    n, (nx, nu, ny) = 8, (4, 1, 6)
    w = fb.Robot2DWorld(n)
    size = dict(xdot0=nx, x0=nx, u0=nu, y0=ny, A=nx * nx, B=nx * nu, C=ny * nx, D=ny * nu)
    b = {k: np.empty(size[k] * n) for k in size}
    st = np.zeros(n, dtype=np.int32)
    ptrs = [None if k in missing.split(" | ") else _pd(b[k]) for k in ("xdot0", "x0", "u0", "y0", "A", "B", "C", "D")]
    assert fb.lib.fb_linearize_state(w._h, fb.K["FB_LIN_FORWARD"], *ptrs, st.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    import re
    with pytest.raises(fb.FlightBatchError, match="did not write " + re.escape(missing) + " on the device"):
        fb.linear_world(w)
    # a full linearisation afterwards serves
    fb.linearize_state(w)
    fb.linear_world(w).close()
    w.close()


# ---- 6. logging ------------------------------------------------------------------------------------------------------------------------
def test_log_equals_snapshots(fb):
    n = 63
    m = make_lss(fb, 4, 1, 6, n, seed=11, stable=True)
    w = fb.LinearWorld(m)
    w.set_state(m.x0.T + 0.5)
    w.u = m.u0.T + 1.0
    w.log_configure(every=10, capacity=16, y=(1, "y4"), x=("x2",))
    snaps, times = [], []
    for _ in range(10):
        w.step(10, dt=0.01, steps_per_launch=7)      # (launches are cut at the save instants)
        x = w.x
        w.f_ode()
        y = w.y
        snaps.append(np.stack([y[1], y[4], x[2]]))
        times.append(w.t)
    t, data = w.log_read()
    assert data.shape == (10, 3, n) and np.array_equal(data, np.stack(snaps))
    assert np.allclose(t, times, rtol=0, atol=1e-12) and np.allclose(t, 0.1 * np.arange(1, 11), rtol=0, atol=1e-12)
    w.close()


# ---- 7. verbs that do not apply --------------------------------------------------------------------------------------------------------
def test_verbs_of_other_models_are_refused_and_change_nothing(fb):
    n = 5
    m = make_lss(fb, 5, 2, 3, n, seed=2, stable=True)
    w, twin = fb.LinearWorld(m), fb.LinearWorld(m)
    L, h = fb.lib, w._h
    buf = np.zeros((64, n))
    i32 = np.zeros(8, dtype=np.int32)
    pi = i32.ctypes.data_as(C.POINTER(C.c_int32))
    dims = (C.c_int64 * 1)(16)
    calls = {
        "fb_trim": lambda: L.fb_trim(h, _pd(buf), _pd(buf), None, None),
        "fb_set_env": lambda: L.fb_set_env(h, _pd(buf)),
        "fb_set_table": lambda: L.fb_set_table(h, fb.K["FB_TABLE_AERO"], buf.ctypes.data_as(C.c_void_p), dims, 1),
        "fb_set_table(scenario)": lambda: L.fb_set_table(h, fb.K["FB_TABLE_SCENARIO"], buf.ctypes.data_as(C.c_void_p), dims, 1),
        "fb_set_ctl_inputs": lambda: L.fb_set_ctl_inputs(h, _pd(buf)),
        "fb_scenario_configure": lambda: L.fb_scenario_configure(h, 1),
        "fb_linearize_dims": lambda: L.fb_linearize_dims(h, pi, pi, pi),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert b"LinearizedSS" in L.fb_last_error(), (name, L.fb_last_error())
    x_before = w.x
    assert L.fb_f_step(h) == 0 and L.fb_f_periodic(h) == 0               # @no_step, @no_periodic
    assert np.array_equal(w.x, x_before) and np.array_equal(w.u, m.u0.T)
    for v in (w, twin):
        v.u = m.u0.T + 1.0
        v.step(50, dt=0.01, steps_per_launch=50)
    assert np.array_equal(w.x, twin.x) and not np.array_equal(w.x, x_before)
    w.close(); twin.close()
