"""fb_lss_poles (flightbatch.poles): the poles of a batch of LinearizedSS models on the device, pinned by

  1. LAPACK on random systems of every group size and batch edge, through the numpy restatement of the kernel's algorithm
     (tests/poles_prototype.py; tests/test_poles_host.py holds the prototype itself to LAPACK first);
  2. the badly scaled system that only balancing gets right, among ordinary neighbours;
  3. the exact cases (zero columns, deflation at once, pairs on the imaginary axis, triangular matrices), value for value;
  4. position independence and reproducibility, bit for bit, and the handle left as it was;
  5. non-finite input, flagged in place among healthy neighbours;
  6. the two tables the reference's robot2d design notebook stores, from linearize on the device to dampreport;
  7. Cessna172Xv2(NED) at the 28 design nodes, the full model and the design subsystems, by backward error;
  8. the loops fb_lqr designs, checked for stability;
  9. the refusals of the C ABI on a live device;
 10. examples/modes_envelope.py.

The shared metric: device and reference poles matched by scipy.optimize.linear_sum_assignment on |pole_i - mu_j|, dev = worst matched
distance / max|mu|. The shared bound: the device differs from the prototype in FMA contraction and <= 1-ulp division only, so it may deviate
from LAPACK ten times as far as the prototype does over the same systems, with the project's fp64 parity bound of 1e-11 as the floor."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import poles_prototype as proto
import reference_fixtures as rf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR, MARGIN = 1e-11, 10.0
NMAX = 130


@functools.lru_cache(maxsize=None)
def _reference(nx):
    """the 130 systems of one size with the prototype's and LAPACK's poles (computed once, read only)"""
    A = proto.systems(nx, NMAX)
    lam, iters, status = proto.poles_batch(A)
    mu = np.array([np.linalg.eigvals(a) for a in A])
    for a in (A, lam, iters, status, mu):
        a.setflags(write=False)
    return A, lam, iters, mu


def _world(fb, A):
    A = np.asarray(A, dtype=np.float64)
    return fb.LinearWorld(fb.design_model(A, np.ones((A.shape[0], A.shape[1], 1))))


def _poles(fb, A):
    w = _world(fb, A)
    res = fb.poles(w)
    w.close()
    return res


def _conjugates_exact(lam):
    """every pole with Im > 0 has a partner with the same Re bits and -Im, and as many poles have Im < 0"""
    up, dn = lam[lam.imag > 0], lam[lam.imag < 0]
    return len(up) == len(dn) and sorted(zip(up.real, up.imag)) == sorted(zip(dn.real, -dn.imag))


# ---- 1. every size and batch edge against LAPACK -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, NMAX])
@pytest.mark.parametrize("nx", proto.NX_ALL)
def test_random_systems_against_lapack(fb, nx, n, capsys):
    A, lam_p, it_p, mu = _reference(nx)
    w = _world(fb, A[:n])
    assert np.array_equal(w.model()[0], A[:n])
    res = fb.poles(w)
    w.close()
    assert res.poles.shape == (n, nx) and res.poles.dtype == np.complex128 and res.iters.shape == res.status.shape == (n,)
    d, p = proto.batch_dev(res.poles, mu[:n]), proto.batch_dev(lam_p[:n], mu[:n])
    med, med_p = float(np.median(res.iters)), float(np.median(it_p[:n]))
    with capsys.disabled():
        print(f"\n[fb_lss_poles vs LAPACK] nx {nx:2d} x {n:3d}: {d:.2e} (prototype {p:.2e})  sweeps {res.iters.min()} / {med:g} / {res.iters.max()} "
              f"(prototype {it_p[:n].min()} / {med_p:g} / {it_p[:n].max()})  status {np.unique(res.status)}", end="")
    assert (res.status == 0).all()
    assert d <= max(MARGIN * p, FLOOR)
    for i in range(n):
        assert (res.poles[i].imag > 0).sum() == (mu[i].imag > 0).sum(), i
        assert _conjugates_exact(res.poles[i]), i
        assert proto.sort_rule_holds(res.poles[i]), i
    assert (res.iters <= 30 * nx).all()
    assert abs(med - med_p) <= 1
    assert res.stable.shape == (n,) and np.array_equal(res.stable, res.poles.real.max(axis=1) < 0)
    assert np.array_equal(res.wn, np.abs(res.poles)) and np.array_equal(res.tau, -1.0 / res.poles.real)


# ---- 2. balancing ------------------------------------------------------------------------------------------------------------------------
def test_the_badly_scaled_system_among_ordinary_neighbours(fb, capsys):
    A0, As = proto.badly_scaled()
    mu = np.linalg.eigvals(A0)
    A = np.array(proto.systems(16, 8))
    A[3] = As
    res = _poles(fb, A)
    d, p = proto.match_dev(res.poles[3], mu), proto.match_dev(proto.poles(As)[0], mu)
    raw = proto.match_dev(proto.poles(As, balancing=False)[0], mu)
    with capsys.disabled():
        print(f"\n[fb_lss_poles, badly scaled] {d:.2e} of eig(A) (prototype {p:.2e}; without balancing {raw:.2e})", end="")
    assert (res.status == 0).all()
    assert d <= max(MARGIN * p, FLOOR)
    ref = _reference(16)
    keep = [i for i in range(8) if i != 3]
    assert proto.batch_dev(res.poles[keep], ref[3][keep]) <= max(MARGIN * proto.batch_dev(ref[1][keep], ref[3][keep]), FLOOR)


# ---- 3. exact cases ----------------------------------------------------------------------------------------------------------------------
def test_exact_cases(fb):
    for A, want in proto.exact_cases():
        res = _poles(fb, np.array([A, A]))
        assert (res.status == 0).all(), (A, res.status)
        for k in (0, 1):
            assert np.array_equal(res.poles[k].real, want.real) and np.array_equal(res.poles[k].imag, want.imag), (A, res.poles[k], want)
    res = _poles(fb, np.array([[[-2.5]], [[0.0]], [[3.0]]]))
    assert np.array_equal(res.poles, np.array([[-2.5 + 0j], [0j], [3.0 + 0j]])) and (res.iters == 0).all() and (res.status == 0).all()
    assert np.array_equal(res.stable, [True, False, False])


# ---- 4. position independence, reproducibility, and nothing written on the handle -------------------------------------------------------
def test_bitwise_independent_of_position_and_repeatable(fb):
    A = proto.systems(11, NMAX)
    rng = np.random.default_rng(4)
    x0 = rng.standard_normal((NMAX, 11))
    w = fb.LinearWorld(fb.design_model(A, np.ones((NMAX, 11, 1)), x0=x0))
    w.u = rng.standard_normal((1, NMAX))
    w.step(7, dt=1e-3)
    w.sync()
    before = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model())
    first = fb.poles(w)
    again = fb.poles(w)
    after = (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model())
    w.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[2] == pytest.approx(7e-3)
    assert (first.status == 0).all()
    bits = lambda z: np.ascontiguousarray(z).view(np.uint64)
    same = lambda p, q, sel=slice(None): (np.array_equal(bits(p.poles[sel]), bits(q.poles)) and np.array_equal(p.iters[sel], q.iters)
                                          and np.array_equal(p.status[sel], q.status))
    assert same(first, again)
    assert same(first, _poles(fb, A[::-1]), slice(None, None, -1))
    pick = np.array([129, 0, 64, 63, 17, 1, 100])
    assert same(first, _poles(fb, A[pick]), pick)


# ---- 5. non-finite input -------------------------------------------------------------------------------------------------------------------
def test_non_finite_systems_are_flagged_in_place(fb):
    A = np.array(proto.systems(5, 65))
    A[7, 2, 3] = np.nan
    A[64, 4, 0] = np.inf
    w = _world(fb, A)
    re, im = np.empty(5 * 65), np.empty(5 * 65)
    iters, status = np.empty(65, dtype=np.int32), np.empty(65, dtype=np.int32)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert fb.lib.fb_lss_poles(w._h, pd(re), pd(im), pi(iters), pi(status)) == 0, fb.lib.fb_last_error()
    assert fb.lib.fb_lss_poles(w._h, None, None, None, None) == 0          # (any output may be NULL)
    res = fb.poles(w)
    w.close()
    assert np.array_equal(res.status, status) and np.array_equal(res.iters, iters)
    assert np.array_equal(res.poles.real.T.reshape(-1), re, equal_nan=True) and np.array_equal(res.poles.imag.T.reshape(-1), im, equal_nan=True)
    bad = np.zeros(65, dtype=bool)
    bad[[7, 64]] = True
    assert np.array_equal(res.status, np.where(bad, proto.NOT_FINITE, 0))
    assert np.isnan(res.poles[bad].real).all() and np.isnan(res.poles[bad].imag).all() and (res.iters[bad] == 0).all()
    assert np.isfinite(res.poles[~bad].real).all() and not res.stable[bad].any()
    healthy = _poles(fb, A[~bad])
    assert (healthy.status == 0).all()
    assert np.array_equal(res.poles[~bad].view(np.uint64), healthy.poles.view(np.uint64)) and np.array_equal(res.iters[~bad], healthy.iters)


# ---- 6. the notebook's tables, end to end ----------------------------------------------------------------------------------------------------
def test_the_notebooks_tables_from_linearize_to_dampreport(fb, capsys):
    w = fb.Robot2DWorld(3)
    lss = fb.linearize(w, None, scheme="forward")
    lw = fb.linear_world(w)
    w.close()
    res = fb.poles(lw)
    lw.close()
    assert (res.status == 0).all() and np.array_equal(res.poles, np.broadcast_to(res.poles[:1], res.poles.shape))
    proto.assert_matches_table(res.poles[0], "open_loop")
    header, lines, _ = proto.table_rows("open_loop")
    assert proto.report_with_zero_snapped(fb, res.poles[0]) == header + lines
    # the closed velocity loop, built on the host from the device's A, B and the h5 gains (C_v picks v)
    Acl = proto.velocity_loop(lss.A[0], lss.B[0])
    cl = _poles(fb, Acl[None])
    assert (cl.status == 0).all()
    proto.assert_matches_table(cl.poles[0], "velocity_loop")
    header, lines, _ = proto.table_rows("velocity_loop")
    assert proto.report_with_zero_snapped(fb, cl.poles[0]) == header + lines
    with capsys.disabled():
        print("\n[fb_lss_poles, Robot2D] open loop " + " ".join(f"{v:+.6g}" for v in res.poles[0].real) + "; velocity loop "
              + " ".join(f"{v:+.6g}" for v in cl.poles[0].real) + f"; stable {bool(res.stable[0])} / {bool(cl.stable[0])}", end="")
    assert not res.stable[0] and not cl.stable[0]      # (the pole at zero: η integrates v)


# ---- 7. the aircraft by backward error ---------------------------------------------------------------------------------------------------------
def _backward(lam, B):
    """max_k sigma_min(B - pole_k I) / ||B||_2"""
    nrm = np.linalg.norm(B, 2)
    eye = np.eye(B.shape[0])
    return max(np.linalg.svd(B - l * eye, compute_uv=False)[-1] for l in lam) / nrm


def test_aircraft_models_by_backward_error(fb, capsys):
    import reference_lqr as rl
    EAS, h, flaps = rf.design_nodes()
    w = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme="onesided2")
    w.close()
    assert lss.success.all() and (lss.status == 0).all()
    iy = [lss.y_labels.index(k) for k in ("EAS", "α", "β")]
    models = [rl.design_model(lss.A[k], lss.B[k], lss.C[k][iy]) for k in range(28)]
    cases = {"full NED model": np.array(lss.A),
             "longitudinal": np.array([rl._sub(*m, rl.LON_FULL, rl.U_LON)[0] for m in models]),
             "lateral": np.array([rl._sub(*m, rl.LAT_RED, rl.U_LAT)[0] for m in models])}
    for name, A in cases.items():
        res = _poles(fb, A)
        assert (res.status == 0).all(), (name, res.status)
        be_dev = be_pro = tr = 0.0
        for k in range(28):
            lam_p, _, st, bal = proto.poles(A[k], full=True)
            assert st == 0
            be_dev, be_pro = max(be_dev, _backward(res.poles[k], bal)), max(be_pro, _backward(lam_p, bal))
            tr = max(tr, abs(res.poles[k].sum() - np.trace(A[k])) / np.abs(np.diag(A[k])).sum())
            assert _conjugates_exact(res.poles[k]) and proto.sort_rule_holds(res.poles[k])
        with capsys.disabled():
            print(f"\n[fb_lss_poles, Cessna172Xv2 {name}] nx {A.shape[1]:2d} x 28: backward error {be_dev:.2e} (prototype {be_pro:.2e}); "
                  f"|sum poles - tr A| / sum|a_ii| {tr:.2e}; sweeps {res.iters.min()} - {res.iters.max()}; unstable nodes {int((~res.stable).sum())}", end="")
        assert be_dev <= max(MARGIN * be_pro, 1e-13), (name, be_dev, be_pro)
        assert tr <= 1e-11, (name, tr)


# ---- 8. design, then check ------------------------------------------------------------------------------------------------------------------------
def test_designed_loops_are_stable_and_open_loops_are_judged_as_numpy_judges_them(fb, capsys):
    import lqr_prototype as lq
    A, B, Q, R = lq.systems(8, 2, NMAX)
    lss = fb.design_model(A, B)
    w = fb.LinearWorld(lss)
    K = fb.lqr(w, Q, R).K
    op = fb.poles(w)
    w.close()
    cl = fb.closed_loop(lss, K)
    lw = fb.LinearWorld(cl)
    res = fb.poles(lw)
    lw.close()
    mu = np.array([np.linalg.eigvals(a) for a in cl.A])
    pr = proto.poles_batch(cl.A)[0]
    worst = np.abs(res.poles.real.max(axis=1) - mu.real.max(axis=1)) / np.abs(mu).max(axis=1)
    worst_p = np.abs(pr.real.max(axis=1) - mu.real.max(axis=1)) / np.abs(mu).max(axis=1)
    mu_open = np.array([np.linalg.eigvals(a).real.max() for a in A])
    with capsys.disabled():
        print(f"\n[fb_lss_poles after fb_lqr] 130 (8, 2) loops: stable {int(res.stable.sum())}; max Re pole vs numpy {worst.max():.2e} "
              f"(prototype {worst_p.max():.2e}); open loops numpy calls unstable {int((mu_open > 0).sum())}, of them stable here "
              f"{int(op.stable[mu_open > 0].sum())}", end="")
    assert (res.status == 0).all() and res.stable.all()
    assert worst.max() <= max(MARGIN * worst_p.max(), FLOOR)
    assert (mu_open > 0).any() and not op.stable[mu_open > 0].any()


# ---- 9. refusals on a live device --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing(fb):
    n = 5
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def launches(h):
        ms, nl = C.c_float(), C.c_int64()
        assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
        assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
        return nl.value

    def call(h, nx):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        re, im = np.empty(nx * n), np.empty(nx * n)
        rc = fb.lib.fb_lss_poles(h, pd(re), pd(im), None, None)
        return rc, fb.lib.fb_last_error(), launches(h)

    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    rc, err, nl = call(ac._h, 20)
    assert rc != 0 and b"fb_lss_poles" in err and b"not a LinearizedSS handle" in err and nl == 0, err
    ac.close()
    h = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 1, 3, n, 0, C.byref(h)) == 0
    rc, err, nl = call(h, 3)
    assert rc != 0 and b"fb_lss_poles" in err and b"no model yet" in err and nl == 0, err
    fb.lib.fb_destroy(h)
    w = _world(fb, proto.systems(3, n))
    rc, err, nl = call(w._h, 3)
    assert rc == 0 and nl == 1, err
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        r = fb.Robot2DWorld(n)
        try:
            fb.poles(r)
        finally:
            r.close()
    w.close()


# ---- 10. the example -------------------------------------------------------------------------------------------------------------------------------
def test_the_modes_envelope_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "modes_envelope.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "short period" in out.stdout and "unstable" in out.stdout
