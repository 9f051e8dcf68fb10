"""fb_linearize / fb_linearize_state (flightbatch.linearization): linearize(vehicle, trim_params) and linearize(f, h, x0, u0) on the device
(FP/aircraftbase.jl:292-334, FP/linearization.jl:55-111, FA/robot2d/robot2d.jl:315-341), pinned by

  1. the Robot2D A, B, C, D the reference's design notebook printed, and the gains it designed from them (robot2d.h5);
  2. the reference's stored LQR gain tables of the Cessna172Xv2 autopilot, redesigned from the device's Jacobians at the 28 nodes;
  3. the same quotients formed on the host from fb_f_ode, point for point, off trim;
  4. the oracle's f_ode under the same scheme;
plus the verb's effect on the handle, its refusals, the status bits and batch-size invariance; Robot2D on distinct robots under both
schemes (the reference held to the oracle's f_ode), partial block requests, and inputs at the bounds of their Ranged types."""
import ctypes as C

import numpy as np
import pytest

import reference_fixtures as rf
from support import clock as _clock

pytestmark = pytest.mark.gpu
W_RATED = 2700 * np.pi / 30
SQRT_EPS = 2.0 ** -26


def _mats(lss, order=(1, 2, 0)):
    return [getattr(lss, k).transpose(*order) for k in "ABCD"]


# ---- 1. Robot2D against the reference's printed matrices -------------------------------------------------------------------------
def test_robot2d_forward_reproduces_the_references_printed_matrices(fb, capsys):
    from reference_fixtures import check_jacobian_and_design
    w = fb.Robot2DWorld(64)
    lss = fb.linearize(w, None, scheme="forward")
    assert lss.A.shape == (64, 4, 4) and lss.B.shape == (64, 4, 1) and lss.C.shape == (64, 6, 4) and lss.D.shape == (64, 6, 1)
    assert lss.x_labels == ("ω", "v", "θ", "η") and lss.u_labels == ("m",)
    for k in "ABCD":
        assert np.array_equal(getattr(lss, k), np.broadcast_to(getattr(lss, k)[:1], getattr(lss, k).shape))
    assert (lss.status == 0).all()
    with capsys.disabled():
        check_jacobian_and_design(lss.A[0], lss.B[0], lss.C[0], lss.D[0], log=lambda s: print("\n[fb_linearize FORWARD] " + s, end=""))
    w.close()


# ---- 2. Cessna172Xv2(NED) against the reference's LQR gain tables -----------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["onesided2", "forward"])
def test_x2_jacobian_reproduces_the_references_lqr_gains(fb, scheme, capsys):
    pytest.importorskip("scipy.linalg")
    import reference_lqr as rl
    EAS, h, flaps = rf.design_nodes()
    w = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme=scheme)
    assert lss.success.all() and (lss.status == 0).all()
    assert lss.x_labels == tuple(rl.X_LABELS) and lss.u_labels == tuple(rl.U_LABELS)
    A, B, Cm, _ = _mats(lss)
    iy = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    with capsys.disabled():
        dev = rl.compare_all(A, B, Cm[iy], log=lambda s: print(f"\n[fb_linearize {scheme}] " + s, end=""))
    worst = max(v for d in dev.values() for v in d.values())
    assert worst <= 5e-6, dev
    # the actuator block comes out of the differences: ṗ = (cmd - p) / τ
    for k in range(4):
        assert np.abs(lss.A[:, 16 + k, 16 + k] + 20.0).max() <= 1e-8 * 20 and np.abs(lss.B[:, 16 + k, k] - 20.0).max() <= 1e-8 * 20
    w.close()


# ---- 3. point for point against fb_f_ode ---------------------------------------------------------------------------------------
def _abi_rows(x2):
    """row of the C ABI's NED state of each x_ss component"""
    if x2:
        return [25, 26, 27, 19, 20, 21, 28, 29, 30, 22, 23, 24, 0, 1, 9, 8, 12, 13, 14, 15]
    return [18, 19, 20, 12, 13, 14, 21, 22, 23, 15, 16, 17, 0, 1, 9, 8]


U_ROWS = [0, 2, 3, 4]            # FB_U_THROTTLE / AILERON / ELEVATOR / RUDDER
CS_ROWS = [2, 34, 3, 35]         # FB_CS_THROTTLE_CMD / AILERON_CMD / ELEVATOR_CMD / RUDDER_CMD
LO = np.array([0.0, -1.0, -1.0, -1.0])


def _y_ss(x2, x, uss, y):
    rows = [y[28], y[29], y[30], y[0], y[1], y[2], y[31], y[32], y[33], y[15], y[16], y[20], x[0], x[1], x[9]]
    rows += [x[9] / W_RATED, x[8]] + [np.clip(x[12 + k], LO[k], 1.0) for k in range(4)] if x2 else [x[8]]
    rows += [y[165], y[166], y[167], y[62], y[63], y[60], y[59], y[34], y[35], y[36], y[38], y[39], -y[36]]
    return np.vstack(rows + [uss[k] for k in range(4)])


def _host_linearize(fb, x2, w, scheme):
    """the scheme applied on the host to fb_f_ode of a second handle: xdot0, y0, A|B, C|D [n, rows, cols]"""
    n = w.n
    rows = _abi_rows(x2)
    nx, nc = len(rows), len(rows) + 4
    x, u, ui, s = w.x, w.u, w.ui, w.s
    uss = np.clip((w.cs[CS_ROWS] if x2 else u[U_ROWS]), LO[:, None], 1.0)
    z = np.vstack([x[rows], uss])
    if scheme == "forward":
        H = np.maximum(SQRT_EPS * np.abs(z), SQRT_EPS)
        mult = (1.0,)
    else:
        H = (z + 1e-6 * np.maximum(np.abs(z), 1.0)) - z
        mult = (1.0, 2.0)
    npt = 1 + nc * len(mult)
    m = n * npt
    X = np.repeat(x[:, None, :], npt, axis=1)
    US = np.repeat(uss[:, None, :], npt, axis=1)
    for j in range(nc):
        for p, c in enumerate(mult):
            pt = 1 + j * len(mult) + p
            zp = z[j] + H[j] if c == 1.0 else z[j] + 2.0 * H[j]
            if j < nx:
                X[rows[j], pt] = zp
            else:
                US[j - nx, pt] = np.clip(zp, LO[j - nx], 1.0)
    w2 = (fb.Cessna172Xv2World if x2 else fb.BatchedWorld)(m, kinematics="NED")
    w2.x = X.reshape(x.shape[0], m)
    w2.s = np.repeat(s[:, None, :], npt, axis=1).reshape(s.shape[0], m)
    U = np.repeat(u[:, None, :], npt, axis=1)
    if x2:
        cs = np.repeat(w.cs[:, None, :], npt, axis=1)
        for k in range(4):
            cs[CS_ROWS[k]] = US[k]
        w2.cs = cs.reshape(cs.shape[0], m)
    else:
        for k in range(4):
            U[U_ROWS[k]] = US[k]
    w2.u = U.reshape(u.shape[0], m)
    w2.ui = np.repeat(ui[None, :], npt, axis=0).reshape(m)
    xd = np.zeros((x.shape[0], m))
    fb.f_ode(w2, xd)
    Y = w2.y
    w2.close()
    f = np.vstack([xd[rows], _y_ss(x2, X.reshape(x.shape[0], m), US.reshape(4, m), Y)]).reshape(-1, npt, n)
    f0 = f[:, 0]
    J = np.zeros((f.shape[0], nc, n))
    for j in range(nc):
        if scheme == "forward":
            J[:, j] = (f[:, 1 + j] - f0) / H[j]
        else:
            J[:, j] = (-3.0 * f0 + 4.0 * f[:, 1 + 2 * j] - f[:, 2 + 2 * j]) / (2.0 * H[j])
    return f0[:nx].T, f0[nx:].T, J[:nx].transpose(2, 0, 1), J[nx:].transpose(2, 0, 1), z


def _spread_trimmed(fb, x2, n, seed=7):
    rng = np.random.default_rng(seed)
    w = (fb.Cessna172Xv2World if x2 else fb.BatchedWorld)(n, kinematics="NED")
    tp = fb.TrimParameters(EAS=rng.uniform(30, 55, n), h_e=rng.uniform(200, 3000, n), γ_wb_n=rng.uniform(-0.05, 0.05, n),
                           ψ_wb_dot=rng.uniform(-0.05, 0.05, n), flaps=rng.uniform(0, 0.5, n), ψ_nb=rng.uniform(-3, 3, n))
    fb.f_init(w, tp)
    assert w.trim_success.mean() > 0.9
    x = w.x
    rows = _abi_rows(x2)
    for r, s in zip(rows[:9], (0.02, 0.02, 0.02, 0.05, 0.02, 0.05, 0.5, 0.3, 0.3)):
        x[r] += rng.uniform(-s, s, n)
    x[0] += rng.uniform(-0.01, 0.01, n)
    w.x = x
    return w


def _scaled_err(got, want):   # (on purpose not support.state_scale: matrices, each system scaled by its own largest entry)
    scale = np.maximum(np.abs(want).reshape(want.shape[0], -1).max(axis=1), 1e-300)
    return (np.abs(got - want).reshape(want.shape[0], -1).max(axis=1) / scale).max()


@pytest.mark.parametrize("x2", [False, True], ids=["c172s0", "c172x2"])
@pytest.mark.parametrize("scheme", ["onesided2", "forward"])
def test_linearize_state_is_fb_f_ode_differenced(fb, x2, scheme, capsys):
    n = 2048
    w = _spread_trimmed(fb, x2, n)
    x_before, s_before, u_before, st_before = w.x, w.s, w.u, w.status
    lss = fb.linearize_state(w, scheme=scheme)
    # the handle is untouched
    assert np.array_equal(w.x, x_before) and np.array_equal(w.s, s_before) and np.array_equal(w.u, u_before) and np.array_equal(w.status, st_before)
    xd0, y0, AB, CD, z = _host_linearize(fb, x2, w, scheme)
    nx = len(_abi_rows(x2))
    # x0 / u0: exactly the mapped rows
    assert np.array_equal(lss.x0, z[:nx].T) and np.array_equal(lss.u0, z[nx:].T)
    dx = np.abs(lss.xdot0 - xd0).max(axis=1) / np.maximum(np.abs(xd0).max(axis=1), 1e-300)
    dy = np.abs(lss.y0 - y0).max(axis=1) / np.maximum(np.abs(y0).max(axis=1), 1e-300)
    tol = 1e-9 if scheme == "onesided2" else 1e-6
    errs = {k: _scaled_err(got, want) for k, got, want in (("A", lss.A, AB[:, :, :nx]), ("B", lss.B, AB[:, :, nx:]),
                                                          ("C", lss.C, CD[:, :, :nx]), ("D", lss.D, CD[:, :, nx:]))}
    with capsys.disabled():
        print(f"\n[{'Xv2' if x2 else 'Sv0'} {scheme}] ẋ0 / y0 vs fb_f_ode: bit-identical aircraft {np.mean(dx == 0):.3f} / {np.mean(dy == 0):.3f}, "
              f"max rel {dx.max():.1e} / {dy.max():.1e}; A B C D vs host quotients: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()), end="")
    if not x2:
        # Cessna172Sv0: the evaluation rounds as k_f_ode's, bit for bit (lin_kernels.hpp, LinSink), and so do the quotients' inputs
        assert (dx == 0).all() and (dy == 0).all()
        assert all(v <= tol for v in errs.values()), errs
    else:
        # Cessna172Xv2: the record rows that fb_f_ode stores and the linearisation does not are contracted differently (fused into their
        # consumers): ẋ0 measured <= 1.4e-13 of its largest entry, y0 2.5e-18; over ONESIDED2's 1e-6 steps that is <= 2.7e-9 of a
        # matrix's largest entry (FORWARD: 7.3e-8, inside its 1e-6). docs/design/linearize.md
        assert dx.max() <= 5e-13 and dy.max() <= 1e-16
        assert all(v <= (1e-8 if scheme == "onesided2" else tol) for v in errs.values()), errs
    w.close()


# ---- 4. against the oracle ---------------------------------------------------------------------------------------------------------
def test_onesided2_matches_the_oracle(fb, oracle, capsys):
    import reference_lqr as rl
    from reference_fixtures import design_trim_parameters_packed as _trim_parameters_packed   # noqa: F401  (the same node set as the LQR pins)
    n = 256
    w = _spread_trimmed(fb, False, n, seed=3)
    lss = fb.linearize_state(w, scheme="onesided2")
    x24, u, ui, s = w.x, w.u, w.ui, w.s
    x27 = np.zeros((27, n))
    x27[:12] = x24[:12]; x27[12:18] = x24[12:18]; x27[21:27] = x24[18:24]
    assert oracle.lib.fo_set_kinematics(2) == 0
    try:
        env = oracle.default_env()

        def f_ode(X, U):
            m = X.shape[1]
            xd, y, st = oracle.f_ode(X, U, np.tile(ui, m // n), np.tile(s, (1, m // n)), env)
            return xd, y
        A, B, Cy = rl.linearize(f_ode, x27, u)   # the actuator-free 16 columns of A: rows / columns 0-15; its u columns are actuator positions
    finally:
        oracle.lib.fo_set_kinematics(0)
    got = lss.A.transpose(1, 2, 0)
    err = np.abs(got - A[:16, :16]).max(axis=(0, 1)) / np.abs(A[:16, :16]).max(axis=(0, 1))
    iy = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    errc = np.abs(lss.C.transpose(1, 2, 0)[iy] - Cy[:, :16]).max(axis=(0, 1)) / np.abs(Cy[:, :16]).max(axis=(0, 1))
    # B: Sv0's inputs act through the same surfaces the Xv0 actuator positions set (rl: columns 16-19 of A)
    errb = np.abs(lss.B.transpose(1, 2, 0) - A[:16, 16:]).max(axis=(0, 1)) / np.abs(A[:16, 16:]).max(axis=(0, 1))
    with capsys.disabled():
        print(f"\n[oracle, onesided2] A {err.max():.1e}  B {errb.max():.1e}  C(EAS, α, β) {errc.max():.1e}", end="")
    assert err.max() <= 1e-6 and errb.max() <= 1e-6 and errc.max() <= 1e-6


# ---- 5. semantics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x2", [False, True], ids=["c172s0", "c172x2"])
def test_linearize_leaves_the_still_air_trim_and_keeps_the_environment(fb, x2):
    n = 64
    W = fb.Cessna172Xv2World if x2 else fb.BatchedWorld
    rng = np.random.default_rng(11)
    tp = fb.TrimParameters(EAS=rng.uniform(35, 50, n), h_e=rng.uniform(300, 2000, n))
    ref = W(n, kinematics="NED")
    fb.f_init(ref, tp)
    w = W(n, kinematics="NED")
    w.set_params(wind_ned=(3.0, -2.0, 0.5), T_sl=300.0)
    env = np.zeros((6, n)); env[0] = 5.0; env[3] = 280.0; env[4] = 100000.0; env[5] = 20.0
    w.env = env
    env_back = w.env
    lss = fb.linearize(w, tp, scheme="forward")
    for k in ("x", "s", "u", "ui", "status") + (("cs", "cu") if x2 else ()):
        assert np.array_equal(getattr(w, k), getattr(ref, k)), k
    assert np.array_equal(lss.success, ref.trim_success) and np.array_equal(lss.cost, ref.trim_cost)
    assert np.array_equal(lss.trim_state, ref.trim_state)
    assert w.has_env and np.array_equal(w.env, env_back)
    assert np.array_equal(w.termination[0], ref.termination[0]) and np.array_equal(w.termination[1], ref.termination[1])
    cnt = C.c_int64()
    fb.lib.fb_get_step_count(w._h, C.byref(cnt))
    assert cnt.value == 0 and fb.lib.fb_time(w._h) == 0.0
    ref.close(); w.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_change_nothing(fb):
    K = fb.K
    n = 8
    for kin in ("WA", "ECEF"):
        w = fb.BatchedWorld(n, kinematics=kin)
        assert fb.lib.fb_linearize_dims(w._h, None, None, None) < 0 and b"NED" in fb.lib.fb_last_error()
        with pytest.raises(fb.FlightBatchError):
            fb.linearize_state(w)
        w.close()
    w = fb.BatchedWorld(n, dtype="f32")
    assert fb.lib.fb_linearize_state(w._h, 0, *([None] * 9)) < 0 and fb.lib.fb_last_error()
    w.close()
    w = fb.BatchedWorld(n, kinematics="NED")
    fb.f_init(w, fb.TrimParameters())
    x, s, u, st = w.x, w.s, w.u, w.status
    assert fb.lib.fb_linearize_state(w._h, 7, *([None] * 9)) < 0 and b"scheme" in fb.lib.fb_last_error()
    ts = np.ascontiguousarray(fb.TrimState(n))
    assert fb.lib.fb_linearize(w._h, None, ts.ctypes.data_as(C.POINTER(C.c_double)), None, None, K["FB_LIN_FORWARD"], *([None] * 9)) < 0
    assert fb.lib.fb_last_error()
    assert np.array_equal(w.x, x) and np.array_equal(w.s, s) and np.array_equal(w.u, u) and np.array_equal(w.status, st)
    w.close()
    assert fb.lib.fb_linearize_state(None, 0, *([None] * 9)) < 0


# ---- 7. throws ---------------------------------------------------------------------------------------------------------------------
def test_an_aircraft_out_of_range_raises_its_bit_and_no_neighbours(fb):
    n = 64
    w = _spread_trimmed(fb, False, n, seed=5)
    x = w.x
    lss_ok = fb.linearize_state(w)
    x[17, 9] = -1000.0 - 1e-9   # h_e just below the altitude floor h_min of geodesy.jl:218-221
    w.x = x
    lss = fb.linearize_state(w)
    assert lss.status[9] & fb.K["FB_ST_ALT_RANGE"]
    others = np.arange(n) != 9
    assert (lss.status[others] == 0).all()
    for k in ("xdot0", "y0", "A", "B", "C", "D"):
        assert np.array_equal(getattr(lss, k)[others], getattr(lss_ok, k)[others]), k
    w.close()


# ---- 8. scale ----------------------------------------------------------------------------------------------------------------------
def test_batch_size_invariance(fb):
    n = 1 << 17
    rng = np.random.default_rng(1)
    tp = fb.TrimParameters(EAS=rng.uniform(30, 55, n), h_e=rng.uniform(100, 3000, n), flaps=rng.uniform(0, 0.5, n))
    w = fb.BatchedWorld(n, kinematics="NED")
    big = fb.linearize(w, tp, scheme="forward")
    ok = big.success
    for k in ("xdot0", "y0", "A", "B", "C", "D"):
        assert np.isfinite(getattr(big, k)[ok]).all(), k
    w.close()
    pick = np.sort(rng.choice(n, 512, replace=False))
    tps = fb.TrimParameters(EAS=tp.EAS[pick], h_e=tp.h_e[pick], flaps=tp.flaps[pick])
    ws = fb.BatchedWorld(512, kinematics="NED")
    small = fb.linearize(ws, tps, scheme="forward")
    for k in ("xdot0", "x0", "u0", "y0", "A", "B", "C", "D", "status", "success", "cost"):
        assert np.array_equal(getattr(small, k), getattr(big, k)[pick]), k
    ws.close()


# ---- 9. Robot2D on distinct robots, both schemes ------------------------------------------------------------------------------------
BLOCKS = ("xdot0", "x0", "u0", "y0", "A", "B", "C", "D")
R2_N = 130
# A's rows 2, 3 (θ̇ = ω, η̇ = v) and C | D's rows 0-4 (y = ω, v, θ, η, u_m) are differences of exact copies of the perturbed components, all
# below 2 in magnitude here. FORWARD: fl(z + h) - z is exact, so the error is the rounding of z + h, <= 2^-53, over h >= 2^-26, plus the
# quotient's own rounding: <= 2^-26 for two ulp of 1 over h. ONESIDED2: z + h is exact by construction; -3 z, its sum with 4 (z + h) and
# fl(z + 2h) round below 8, 4 and 2: <= 2^-51 + 2^-52 + 2^-53 < 2^-50, over 2h >= 2e-6.
R2_EXACT_TOL = {"forward": 2.0 ** -26, "onesided2": 2.0 ** -50 / 2e-6}


def _r2_states(n=R2_N, seed=13):
    """rows 0-4 of n state records: ω, v, θ, η and the motor input u_m, every robot its own"""
    rng = np.random.default_rng(seed)
    return np.vstack([rng.uniform(-s, s, n) for s in (0.5, 0.5, 0.5, 1.0, 0.8)])


def _r2_world(fb, z):
    w = fb.Robot2DWorld(z.shape[1])
    fb.f_init(w, fb.InitParameters())
    x = w.x
    x[:5] = z
    w.x = x
    return w


def _r2_host_linearize(fb, oracle, x, scheme):
    """the scheme applied on the host to fb_f_ode of a second Robot2D handle, which is first held to the oracle's f_ode at every point:
    xdot0 [n, 4], y0 [n, 6], A|B [n, 4, 5], C|D [n, 6, 5]"""
    from support import DEFAULT_VP
    n = x.shape[1]
    z = x[:5]
    if scheme == "forward":
        H = np.maximum(SQRT_EPS * np.abs(z), SQRT_EPS)
        mult = (1.0,)
    else:
        H = (z + 1e-6 * np.maximum(np.abs(z), 1.0)) - z
        mult = (1.0, 2.0)
    npt = 1 + 5 * len(mult)
    m = n * npt
    X = np.repeat(x[:, None, :], npt, axis=1)
    for j in range(5):
        for p, c in enumerate(mult):
            X[j, 1 + j * len(mult) + p] = z[j] + H[j] if c == 1.0 else z[j] + 2.0 * H[j]
    X = np.ascontiguousarray(X.reshape(10, m))
    w2 = fb.Robot2DWorld(m)
    w2.x = X
    xd = np.zeros((4, m))
    fb.f_ode(w2, xd)
    Y = w2.y
    w2.close()
    _D = C.POINTER(C.c_double)
    xdo, vp = np.zeros((4, m)), DEFAULT_VP.copy()
    oracle.lib.fo_robot2d_f_ode(C.c_int64(m), vp.ctypes.data_as(_D), X.ctypes.data_as(_D), xdo.ctypes.data_as(_D))
    pre = np.max(np.abs(xd - xdo) / np.maximum(np.abs(xdo), 1.0))
    assert pre < 1e-12, f"precondition: fb_f_ode is {pre:.3e} from the oracle's f_ode at the points of the reference"
    f = np.vstack([xd, Y[:6]]).reshape(10, npt, n)
    f0 = f[:, 0]
    J = np.zeros((10, 5, n))
    for j in range(5):
        if scheme == "forward":
            J[:, j] = (f[:, 1 + j] - f0) / H[j]
        else:
            J[:, j] = (-3.0 * f0 + 4.0 * f[:, 1 + 2 * j] - f[:, 2 + 2 * j]) / (2.0 * H[j])
    return f0[:4].T, f0[4:].T, J[:4].transpose(2, 0, 1), J[4:].transpose(2, 0, 1)


@pytest.mark.parametrize("scheme", ["forward", "onesided2"])
def test_robot2d_linearize_state_on_distinct_robots(fb, oracle, scheme, capsys):
    n = R2_N
    z = _r2_states()
    w = _r2_world(fb, z)
    x_before, u_before, st_before, clock_before = w.x, w.u, w.status, _clock(fb, w)
    lss = fb.linearize_state(w, scheme=scheme)
    assert np.array_equal(w.x, x_before) and np.array_equal(w.u, u_before) and np.array_equal(w.status, st_before) and _clock(fb, w) == clock_before
    assert (lss.status == 0).all() and lss.A.shape == (n, 4, 4) and lss.B.shape == (n, 4, 1) and lss.C.shape == (n, 6, 4) and lss.D.shape == (n, 6, 1)
    # x0 / u0: exactly the mapped rows; ẋ0 / y0: fb_f_ode's bits
    assert np.array_equal(lss.x0, z[:4].T) and np.array_equal(lss.u0, z[4:].T)
    xd = np.zeros((4, n))
    fb.f_ode(w, xd)
    assert np.array_equal(lss.xdot0, xd.T) and np.array_equal(lss.y0, w.y[:6].T)
    xd0, y0, AB, CD = _r2_host_linearize(fb, oracle, x_before, scheme)
    assert np.array_equal(lss.xdot0, xd0) and np.array_equal(lss.y0, y0)
    tol = 1e-9 if scheme == "onesided2" else 1e-6
    errs = {k: _scaled_err(got, want) for k, got, want in (("A", lss.A, AB[:, :, :4]), ("B", lss.B, AB[:, :, 4:]),
                                                          ("C", lss.C, CD[:, :, :4]), ("D", lss.D, CD[:, :, 4:]))}
    # what the reference's model fixes
    I4 = np.eye(4)
    exact = max(np.abs(lss.A[:, 2:] - I4[:2]).max(), np.abs(lss.C[:, :4] - I4).max(), np.abs(lss.D[:, :4]).max(),
                np.abs(lss.C[:, 4]).max(), np.abs(lss.D[:, 4] - 1.0).max())
    with capsys.disabled():
        print(f"\n[Robot2D {scheme}] A B C D vs host quotients of fb_f_ode: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items())
              + f"; fixed entries within {exact:.1e} (bound {R2_EXACT_TOL[scheme]:.1e})", end="")
    assert all(v <= tol for v in errs.values()), errs
    assert exact <= R2_EXACT_TOL[scheme]
    # neighbours differ (a lane that read another robot's row or column would show against the host, and this is why)
    assert np.abs(lss.A[1:, :2] - lss.A[:-1, :2]).reshape(n - 1, -1).max(axis=1).min() > 0
    w.close()
    # the first robots alone: the same bits (a lone lane, a partial wave)
    for k in (1, 63):
        ws = _r2_world(fb, z[:, :k])
        sub = fb.linearize_state(ws, scheme=scheme)
        for b in BLOCKS + ("status",):
            assert np.array_equal(getattr(sub, b), getattr(lss, b)[:k]), (k, b)
        ws.close()


@pytest.mark.parametrize("scheme", ["forward", "onesided2"])
def test_robot2d_linearize_with_per_robot_init_parameters(fb, scheme):
    n = R2_N
    rng = np.random.default_rng(17)
    ip = fb.InitParameters(u_m=rng.uniform(-0.2, 0.2, n), ω=rng.uniform(-0.05, 0.05, n), η=rng.uniform(-1, 1, n))
    w, ref = fb.Robot2DWorld(n), fb.Robot2DWorld(n)
    lss = fb.linearize(w, ip, scheme=scheme)
    fb.f_init(ref, ip)
    # the world is left as f_init leaves it
    assert np.array_equal(w.x, ref.x) and np.array_equal(w.u, ref.u) and np.array_equal(w.status, ref.status) and _clock(fb, w) == _clock(fb, ref)
    assert np.array_equal(w.x[4], ip.pack(n)[0]) and np.array_equal(w.x[0], ip.pack(n)[1]) and np.array_equal(w.x[3], ip.pack(n)[2])
    want = fb.linearize_state(ref, scheme=scheme)
    for b in BLOCKS + ("status",):
        assert np.array_equal(getattr(lss, b), getattr(want, b)), b
    assert np.abs(lss.B[1:] - lss.B[:-1]).max() > 0 or np.abs(lss.A[1:] - lss.A[:-1]).max() > 0
    w.close(); ref.close()


# ---- 10. partial block requests --------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e77
REQUESTS = (("A", "B"), ("C", "D"), ("xdot0", "x0", "u0", "y0"), ("B", "C"))


def _raw_linearize_state(fb, w, scheme, want=BLOCKS):
    """fb_linearize_state with NULL for every block not in `want`; the host buffers start as the sentinel. Returns them and the status."""
    from flightbatch.linearization import dims
    nx, nu, ny = dims(w)
    n = w.n
    size = dict(xdot0=nx, x0=nx, u0=nu, y0=ny, A=nx * nx, B=nx * nu, C=ny * nx, D=ny * nu)
    b = {k: np.full(size[k] * n, SENTINEL) for k in BLOCKS}
    st = np.full(n, -1, dtype=np.int32)
    _D = C.POINTER(C.c_double)
    ptrs = [b[k].ctypes.data_as(_D) if k in want else None for k in BLOCKS]
    rc = fb.lib.fb_linearize_state(w._h, fb.K["FB_LIN_" + scheme.upper()], *ptrs, st.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, fb.lib.fb_last_error()
    for k in BLOCKS:
        if k in want:
            assert not (b[k] == SENTINEL).any() and np.isfinite(b[k]).all(), k        # written, every element
        else:
            assert (b[k] == SENTINEL).all(), k
    return b, st


def _batch_65(fb, robot):
    return _r2_world(fb, _r2_states(65, seed=19)) if robot else _spread_trimmed(fb, False, 65, seed=23)


@pytest.mark.parametrize("robot", [False, True], ids=["c172s0", "robot2d"])
@pytest.mark.parametrize("scheme", ["forward", "onesided2"])
def test_partial_block_requests_give_the_full_calls_bits(fb, robot, scheme):
    w = _batch_65(fb, robot)
    full, st_full = _raw_linearize_state(fb, w, scheme)
    assert (st_full >= 0).all()
    for want in REQUESTS:
        part, st = _raw_linearize_state(fb, w, scheme, want)
        assert np.array_equal(st, st_full), want
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)
    # and the Python route's reshaping agrees with the raw blocks
    lss = fb.linearize_state(w, scheme=scheme)
    n, nx = w.n, lss.x0.shape[1]
    assert np.array_equal(lss.A, full["A"].reshape(nx, nx, n).transpose(2, 1, 0)) and np.array_equal(lss.x0, full["x0"].reshape(nx, n).T)
    w.close()


@pytest.mark.parametrize("robot", [False, True], ids=["c172s0", "robot2d"])
def test_onesided2_after_forward_on_one_handle(fb, robot):
    """the second call needs more room on the device than the first left (the first points' results of the Cessnas)"""
    w, fresh = _batch_65(fb, robot), _batch_65(fb, robot)
    assert np.array_equal(w.x, fresh.x) and np.array_equal(w.u, fresh.u)
    _raw_linearize_state(fb, w, "forward", ("B",))
    got, st = _raw_linearize_state(fb, w, "onesided2")
    want, st_want = _raw_linearize_state(fb, fresh, "onesided2")
    assert np.array_equal(st, st_want)
    for k in BLOCKS:
        assert np.array_equal(got[k], want[k]), k
    # and back: the larger buffer serves the smaller request
    back, _ = _raw_linearize_state(fb, w, "forward")
    first, _ = _raw_linearize_state(fb, fresh, "forward")
    for k in BLOCKS:
        assert np.array_equal(back[k], first[k]), k
    w.close(); fresh.close()


# ---- 11. inputs at the bounds of their Ranged types --------------------------------------------------------------------------------
AT_BOUND = (3, 40, 17, 63, 21)   # lanes: throttle 1, throttle 1, throttle 0, elevator -1, aileron half a step below 1


@pytest.mark.parametrize("x2", [False, True], ids=["c172s0", "c172x2"])
@pytest.mark.parametrize("scheme", ["onesided2", "forward"])
def test_inputs_at_their_bounds(fb, x2, scheme, capsys):
    n = 64
    w = _spread_trimmed(fb, x2, n)
    plain = fb.linearize_state(w, scheme=scheme)
    h_nominal = SQRT_EPS if scheme == "forward" else 1e-6      # the step of either scheme for |z| <= 1
    v = w.cs if x2 else w.u
    rows = CS_ROWS if x2 else U_ROWS
    v[rows[0], [3, 40]] = 1.0
    v[rows[0], 17] = 0.0
    v[rows[2], 63] = -1.0
    v[rows[1], 21] = 1.0 - h_nominal / 2
    if x2:
        w.cs = v
    else:
        w.u = v
    lss = fb.linearize_state(w, scheme=scheme)
    assert lss.u0[3, 0] == 1.0 and lss.u0[40, 0] == 1.0 and lss.u0[17, 0] == 0.0 and lss.u0[63, 2] == -1.0 and lss.u0[21, 1] == 1.0 - h_nominal / 2
    xd0, y0, AB, CD, z = _host_linearize(fb, x2, w, scheme)
    nx = len(_abi_rows(x2))
    assert np.array_equal(lss.x0, z[:nx].T) and np.array_equal(lss.u0, z[nx:].T)
    tol = (1e-8 if x2 else 1e-9) if scheme == "onesided2" else 1e-6      # test_linearize_state_is_fb_f_ode_differenced's
    errs = {k: _scaled_err(got, want) for k, got, want in (("A", lss.A, AB[:, :, :nx]), ("B", lss.B, AB[:, :, nx:]),
                                                          ("C", lss.C, CD[:, :, :nx]), ("D", lss.D, CD[:, :, nx:]))}
    at = list(AT_BOUND)
    errs_at = {k: _scaled_err(got[at], want[at]) for k, got, want in (("B", lss.B, AB[:, :, nx:]), ("D", lss.D, CD[:, :, nx:]))}
    with capsys.disabled():
        print(f"\n[{'Xv2' if x2 else 'Sv0'} {scheme}, inputs at bounds] vs host quotients: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items())
              + "; the five lanes at a bound: " + "  ".join(f"{k} {v:.1e}" for k, v in errs_at.items()), end="")
    assert all(e <= tol for e in errs.values()), errs
    # an input at its upper bound cannot be raised: every point is the baseline, and FORWARD's quotient (f(z) - f(z)) / h is exactly 0, on
    # the host and on the device (ONESIDED2's -3 f + 4 f - f rounds, so its column is held to the host's above and no further)
    if scheme == "forward":
        for lane in (3, 40):
            assert (AB[lane, :, nx] == 0).all() and (CD[lane, :, nx] == 0).all()
            assert (lss.B[lane, :, 0] == 0.0).all() and (lss.D[lane, :, 0] == 0.0).all(), lane
    # at a lower bound the step is free: the column is the host's and is not empty
    for lane, k in ((17, 0), (63, 2)):
        for got, want in ((lss.B[lane, :, k], AB[lane, :, nx + k]), (lss.D[lane, :, k], CD[lane, :, nx + k])):
            assert np.abs(got - want).max() <= tol * max(np.abs(AB[lane]).max(), np.abs(CD[lane]).max())
        assert np.abs(lss.B[lane, :, k]).max() > 0 and np.abs(lss.D[lane, :, k]).max() > 0
    # half a step below the bound: the first point is clipped, the baseline is not, so the column is there but is not the free one
    assert np.abs(lss.B[21, :, 1]).max() > 0 and not np.array_equal(lss.B[21, :, 1], plain.B[21, :, 1])
    # the neighbours know nothing of it
    others = np.setdiff1d(np.arange(n), AT_BOUND)
    for k in BLOCKS + ("status",):
        assert np.array_equal(getattr(lss, k)[others], getattr(plain, k)[others]), k
    w.close()
