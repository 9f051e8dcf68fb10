"""Every instance of the Model(lss) kernels that lss_with_group (csrc/fb_lss.inc) can launch, stepped on the device.

AN INSTANCE ADDED TO `lss_with_group` GETS A ROW HERE (tests/test_lss_host.py::test_lss_and_lqr_kernels_are_in_the_library pins the set in the
code object and points to this table):

    kernel                 nx       exchange                                 stepped here with nx / nu / ny
    k_lss_rk4<4, 0>        1 - 4    LDS panel (the default)                  1/1/1, 4/1/6
    k_lss_rk4<4, 1>        1 - 4    cross-lane reads (FLIGHTBATCH_LSS_EXCHANGE=shfl)    1/1/1, 4/1/6
    k_lss_rk4<8, 0>        5 - 8    LDS panel                                5/2/3, 8/2/3
    k_lss_rk4<8, 1>        5 - 8    cross-lane reads                         5/2/3, 8/2/3
    k_lss_rk4<16, 0>       9 - 16   LDS panel                                9/3/17, 16/4/33
    k_lss_rk4<16, 1>       9 - 16   cross-lane reads                         9/3/17, 16/4/33
    k_lss_rk4<32, 0>       17 - 32  LDS panel                                17/4/5, 32/8/64
    k_lss_rk4<32, 1>       17 - 32  cross-lane reads                         17/4/5, 32/8/64
    k_lss_f_ode<4>         1 - 4    LDS panel (always)                       tests/test_gpu_lss.py::SHAPES: 1/1/1, 4/1/6
    k_lss_f_ode<8>         5 - 8                                             5/2/3, 8/2/3
    k_lss_f_ode<16>        9 - 16                                            9/3/17, 16/4/33
    k_lss_f_ode<32>        17 - 32                                           17/4/5, 20/4/38, 32/8/64

Each group size is stepped at its smallest nx (G - nx padding lanes, for G = 4: three of four) and at nx = G (none). Reference and bound are
those of tests/test_gpu_lss.py: the same RK4 in np.longdouble, 1000 steps of dt = 0.01 with an input step after step 100, scaled error
<= 1e-11 with scale max(|x|, 1), after the precondition that numpy fp64 stays within 1e-13 of the longdouble run. The two exchanges perform the
same operations in the same order (acc = fma(a[c], dz_c, acc), c ascending), so they have to agree bit for bit; `exchange` makes every
world created under it prove which one it steps with (LinearWorld.exchange, fb_lss_exchange)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from support import (LSS_DT as DT, LSS_EXCHANGE_VAR as VAR, LSS_EXCHANGES as EXCHANGES, LSS_N_TRAJ as N_TRAJ, LSS_NSTEPS as NSTEPS, clock as _clock, exchange,
                     lss_run_device as run_device, make_lss, pd as _pd, traj_case)

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (4, 1, 6), (5, 2, 3), (8, 2, 3), (9, 3, 17), (16, 4, 33), (17, 4, 5), (32, 8, 64)]
_shape_id = lambda s: "%d-%d-%d" % s
BLOCKS = ("xdot0", "x0", "u0", "y0", "A", "B", "C", "D")


def first(case, k):
    """the first k systems of a trajectory case (model, start, inputs)"""
    m, xs, ua, ub = case[:4]
    return dataclasses.replace(m, **{b: getattr(m, b)[:k] for b in BLOCKS}), xs[:k], ua[:k], ub[:k]


_device = {}


def device_run(fb, shape, name):
    """the 130 systems of a shape after 1000 steps at 50 steps per launch under one exchange: run once, shared, never modified"""
    if (shape, name) not in _device:
        with exchange(name):
            _device[shape, name] = run_device(fb, traj_case(fb, shape), 50)
    return _device[shape, name]


def test_the_context_manager_selects_and_restores(fb):
    before = os.environ.get(VAR)
    m = make_lss(fb, 3, 1, 2, 5, seed=1)
    for name in EXCHANGES:
        with exchange(name):
            w = fb.LinearWorld(m)
            assert w.exchange == name
            w.close()
        assert os.environ.get(VAR) == before
    # the verb works before a model is set, and says which handle it wants
    h, xch = C.c_void_p(), C.c_int32(-1)
    with exchange("shfl"):
        assert fb.lib.fb_lss_create(3, 1, 2, 5, 0, C.byref(h)) == 0
    assert fb.lib.fb_lss_exchange(h, C.byref(xch)) == 0 and xch.value == 1
    assert fb.lib.fb_lss_exchange(h, None) != 0 and b"fb_lss_exchange" in fb.lib.fb_last_error()
    assert fb.lib.fb_destroy(h) == 0
    r = fb.Robot2DWorld(4)
    xch.value = -1
    assert fb.lib.fb_lss_exchange(r._h, C.byref(xch)) != 0 and b"fb_lss_exchange" in fb.lib.fb_last_error() and xch.value == -1
    r.close()
    w = fb.LinearWorld(m)   # (outside: whatever the environment says, the panel unless it says shfl)
    assert w.exchange == ("shfl" if before == "shfl" else "panel")
    w.close()


# ---- 1. every stepper instance against the longdouble RK4, and against its twin -------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_every_stepper_instance_against_longdouble_rk4(fb, shape, capsys):
    case = traj_case(fb, shape)
    x_ld, x_64 = case[4], case[5]
    scale = np.maximum(np.abs(x_ld), 1.0).astype(np.float64)
    pre = float((np.abs(x_64 - x_ld).astype(np.float64) / scale).max())
    assert pre <= 1e-13, f"precondition: numpy fp64 is {pre:.3e} from the longdouble RK4 (change the inputs, not the number)"
    x = {name: device_run(fb, shape, name) for name in EXCHANGES}
    err = {name: float((np.abs(x[name] - x_ld).astype(np.float64) / scale).max()) for name in EXCHANGES}
    with capsys.disabled():
        print(f"\n[lss rk4 {shape} n={N_TRAJ}, {NSTEPS} steps] scaled error vs longdouble: numpy fp64 {pre:.3e}, panel {err['panel']:.3e}, "
              f"shfl {err['shfl']:.3e}, same bits: {np.array_equal(x['panel'], x['shfl'])}", end="")
    for name in EXCHANGES:
        assert x[name].shape == (N_TRAJ, shape[0]) and err[name] <= 1e-11, (name, err)
    assert np.array_equal(x["panel"], x["shfl"])


# ---- 2. launch partition, both exchanges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXCHANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_launch_partition_gives_the_same_bits(fb, shape, name):
    case = traj_case(fb, shape)
    ref = device_run(fb, shape, name)
    with exchange(name):
        for spl in (1, 7):
            assert np.array_equal(run_device(fb, case, spl), ref), spl
        assert np.array_equal(run_device(fb, case, 50, cuts=([1, 36, 63], [450, 13, 437])), ref)
        assert np.array_equal(run_device(fb, case, 7, cuts=([99, 1], [3] * 300)), ref)


# ---- 3. batch edges: a lone group in a wave, a partial wave, the tail block; position independence ------------------------------------
@pytest.mark.parametrize("name", EXCHANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_the_first_systems_alone_give_the_same_bits(fb, shape, name):
    case = traj_case(fb, shape)
    ref = device_run(fb, shape, name)
    with exchange(name):
        for k in (1, 63):
            x = run_device(fb, first(case, k), 50)
            assert x.shape == (k, shape[0]) and np.array_equal(x, ref[:k]), k


# ---- 4. fb_lss_set_model on a handle that has stepped -----------------------------------------------------------------------------------
def _set_model(fb, w, m):
    from flightbatch.lss import pack_model
    b = pack_model(m)
    assert fb.lib.fb_lss_set_model(w._h, *[_pd(b[k]) for k in BLOCKS]) == 0, fb.lib.fb_last_error()


@pytest.mark.parametrize("name", EXCHANGES)
@pytest.mark.parametrize("shape", [(5, 2, 3), (32, 8, 64)], ids=_shape_id)
def test_a_model_replaced_on_a_stepped_handle(fb, shape, name):
    nx, nu, ny = shape
    n, every = 63, 10
    m1 = make_lss(fb, nx, nu, ny, n, seed=100 + nx, stable=True)
    m2 = make_lss(fb, nx, nu, ny, n, seed=200 + nx, stable=True)
    rng = np.random.default_rng(nx)
    xs, du = m2.x0 + rng.standard_normal((n, nx)), rng.standard_normal((n, nu))
    log = dict(every=every, capacity=16, y=(0, ny - 1), x=(0, nx - 1))
    with exchange(name):
        w, fresh = fb.LinearWorld(m1), fb.LinearWorld(m2)
    w.log_configure(**log)
    fresh.log_configure(**log)
    w.set_state(m1.x0.T + 0.5)
    w.u = m1.u0.T + 1.0
    w.step(37, dt=DT, steps_per_launch=7)
    w.sync()
    assert _clock(fb, w) == (pytest.approx(37 * DT, abs=1e-12), 37) and len(w.log_read()[0]) == 3 and not np.array_equal(w.x, m1.x0.T)
    _set_model(fb, w, m2)
    # Modeling.X(lss) = copy(x0), U = copy(u0); the clock and the step count restart
    assert np.array_equal(w.x, m2.x0.T) and np.array_equal(w.u, m2.u0.T)
    assert _clock(fb, w) == (0.0, 0)
    assert (w.status == 0).all()
    fresh.set_params(dt=DT)
    assert fb.lib.fb_set_steps_per_launch(fresh._h, 7) == 0
    # the same start and inputs on both, by plain assignment (the clocks stay where they are), then the same calls
    for v in (w, fresh):
        v.x = xs.T
        v.u = m2.u0.T + du.T
    taken = []
    for k in (3, 6, 1, 40):        # 37 + 3 = 40: a handle whose log still counted from its first model would save here
        for v in (w, fresh):
            v.step(k)
        taken.append(len(w.log_read()[0]) - 3)
        assert np.array_equal(w.x, fresh.x), k
    assert taken == [0, 0, 1, 5], taken
    assert _clock(fb, w) == _clock(fb, fresh) and _clock(fb, w)[1] == 50
    (tw, dw), (tf, df) = w.log_read(), fresh.log_read()
    assert dw.shape == (8, 4, n) and df.shape == (5, 4, n)
    assert np.array_equal(dw[3:], df) and np.array_equal(tw[3:], tf) and np.allclose(tf, every * DT * np.arange(1, 6), rtol=0, atol=1e-12)
    assert np.isfinite(dw).all() and not np.array_equal(df[0], df[-1])
    w.close(); fresh.close()
