"""Discrete PID design on the device, host side (no GPU compute; docs/design/linearize.md, "Discrete PID design on the device"):

  1. fb_lss_dpid_metrics is declared, exported, bound and wrapped; the kernels of namespace fbu are exactly the three instances of
     k_dpid_metrics, each with 0 B of scratch and the one exchange panel (512 B) of LDS; header, kernel and prototype agree on the
     constants; the refusals that need no device;
  2. the numpy restatement of the kernel (tests/dpid_prototype.py) is held to the exact side (a literal scalar transcription of the law,
     numpy.linalg.solve for P(z)) on every case tests/test_gpu_dpid.py uses — the deviations printed here are what the GPU bound multiplies;
  3. C(z) is the transfer function of the law: the recursion driven open-loop with z^k;
  4. the closed loop assembled from build_dpid and the plant, stepped as one matrix, gives the law's samples, and its r -> e response is
     1 / (1 + P C) on the grid;
  5. the continuous limit: the distance to the continuous compensator's metrics shrinks first-order in Ts;
  6. every bounded case is decided: no free_k within 1e-6 of a bound, no e_k within 1e-6 of zero after a clamped tick, so rounding
     cannot change the clamp or halt history and the device's counts must equal the exact side's integers.

Bounds. Prototype against the exact side: the two differ in summation order and in how C(z) is written; over 100 ticks of a stable loop
that is a few hundred ulp on a metric of order one, and ef = |y_N - 1|, a difference from 1 down to 4e-5 here, sees it 1 / ef times
larger: asserted at 1e-10 on every metric, 1e-12 on Ms (elimination with pivoting against LAPACK's, conditions below 1e3)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dpid_prototype as proto
import pid_prototype as pp

pytest.importorskip("scipy.linalg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Ms", "ie", "ef", "iu", "up")
N_TICKS = int(round(proto.T_SIM / proto.TS))


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_bound_and_wrapped(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h"), encoding="utf-8").read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    name = "fb_lss_dpid_metrics"
    assert name in declared and re.search(rf"\bT {name}\b", out)
    assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == 14
    assert set(fb.EXPORTED) == declared
    assert f"(:{name}, lib)" in shim and re.search(r"^function dpid_metrics\(w::LinearWorld", shim, flags=re.M)
    assert list(inspect.signature(fb.dpid_metrics).parameters) == ["world", "points", "u", "y", "settings", "weights", "bounds", "w"]
    assert list(inspect.signature(fb.optimize_dpid).parameters)[:5] == ["world", "u", "y", "data_0", "settings"]
    assert list(inspect.signature(fb.build_dpid).parameters) == ["point", "Ts"]
    assert set(fb.DPIDMetricsResult.__dataclass_fields__) == {"metrics", "cost", "status", "counts"}
    assert fb.dpid.pattern_search is fb.pidopt.pattern_search


def test_the_constants_agree(fb):
    assert tuple(fb.K[k] for k in ("FB_DPID_DIVERGED", "FB_DPID_SINGULAR", "FB_DPID_DIRECT", "FB_DPID_NX_MAX")) == (
        proto.DIVERGED, proto.SINGULAR, proto.DIRECT, proto.NX_MAX) == (1, 2, 4, 31)
    assert (fb.dpid.DIVERGED, fb.dpid.SINGULAR, fb.dpid.DIRECT, fb.dpid.NX_MAX) == (1, 2, 4, 31)
    text = open(os.path.join(ROOT, "flight.jl_amd", "csrc", "dpid_kernels.hpp"), encoding="utf-8").read()
    assert float(re.search(r"constexpr double DPID_MS_MAX = ([0-9.e+]+);", text).group(1)) == proto.MS_MAX == pp.MS_MAX
    assert float(re.search(r"constexpr double DPID_BLOWUP = ([0-9.e+]+);", text).group(1)) == proto.BLOWUP == pp.BLOWUP
    assert "#pragma unroll 1\n    for (int k = 0; k <= N; k++)" in text      # the tick loop is not unrolled


def test_the_three_kernel_instances_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    want = {f"fbu::k_dpid_metrics<{P}>" for P in (8, 16, 32)}
    assert {k for k in ks if k.startswith("fbu::")} == want, sorted(k for k in ks if k.startswith("fbu::"))
    for name in want:
        print(name, ks[name])
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == 64 * 8 and "k_step_" not in name      # one double per lane: the exchange panel
    for P in (8, 16, 32):
        assert f"fbw::k_lss_dfreqresp<{P}>" in ks          # P(z) on the grid: the d verbs' kernel, a second launch site


class _World:
    n, nx, nu, ny = 3, 2, 1, 1
    u_labels, y_labels = ("u",), ("y",)
    _h = None
    Ts = 0.02


def test_refusals_that_need_no_device(fb):
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    w = np.logspace(-1, 1, 5)
    pid, cost, st = np.ones(4), np.empty(1), np.empty(1, dtype=np.int32)
    rc = fb.lib.fb_lss_dpid_metrics(None, 0, 0, w.ctypes.data_as(D), 5, 2.0, None, pid.ctypes.data_as(D), None, 1, None, cost.ctypes.data_as(D), None,
                                    st.ctypes.data_as(I))
    err = fb.lib.fb_last_error()
    assert rc != 0 and b"null handle" in err and b"fb_lss_dpid_metrics" in err, err
    world = _World()
    ok = np.tile(np.array([1.0, 0.5, 0.0, 0.01]), (3, 2, 1))
    for bad, msg in ((np.ones((3, 2, 3)), "points must be"), (np.ones((2, 2, 4)), "points must be"), (np.ones((3, 65, 4)), "m = 65"),
                     (np.ones((3, 0, 4)), "m = 0")):
        with pytest.raises(ValueError, match=msg):
            fb.dpid_metrics(world, bad)
    for tf in (-0.01, np.nan, np.inf):
        p = ok.copy(); p[1, 1, 3] = tf
        with pytest.raises(ValueError, match="τ_f must be finite and not negative"):
            fb.dpid_metrics(world, p)
    with pytest.raises(ValueError, match="input index 1"):
        fb.dpid_metrics(world, ok, u=1)
    for wt in (np.ones(4), [1, 1, 1, 1, -1], np.zeros(5)):
        with pytest.raises(ValueError, match="weights"):
            fb.dpid_metrics(world, ok, weights=wt)
    for bnd in ((1.0, 1.0), (2.0, -2.0), (np.nan, 1.0), (-1.0, np.nan), (np.inf, np.inf), (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match="bounds"):
            fb.dpid_metrics(world, ok, bounds=bnd)
    with pytest.raises(fb.FlightBatchError, match="LinearWorld"):      # (τ_f = 0 and one-sided bounds pass: the next check is the world's)
        zero = ok.copy(); zero[..., 3] = 0.0
        fb.dpid_metrics(world, zero, bounds=(-np.inf, 1.0))
    S, P = fb.Settings, fb.PIDData
    with pytest.raises(ValueError, match="lower <= upper"):
        fb.optimize_dpid(world, settings=S(lower_bounds=P(k_p=2.0, k_i=0, k_d=0, τ_f=0.01), upper_bounds=P(k_p=1.0, k_i=1, k_d=1, τ_f=0.01)))
    with pytest.raises(ValueError, match="τ_f"):
        fb.optimize_dpid(world, settings=S(lower_bounds=P(k_p=0, k_i=0, k_d=0, τ_f=-0.1), upper_bounds=P(k_p=1.0, k_i=1, k_d=1, τ_f=0.01)))
    with pytest.raises(ValueError, match="data_0"):
        fb.optimize_dpid(world, data_0=np.ones((2, 4)))
    for bad in ((1.0, 0.0, 0.0, -1.0), (1.0, 0.0, 0.0, np.nan)):
        with pytest.raises(ValueError, match="τ_f"):
            fb.build_dpid(bad, 0.02)
    with pytest.raises(ValueError, match="Ts"):
        fb.build_dpid((1.0, 0.0, 0.0, 0.01), 0.0)


# ---- 2. the prototype against the exact side on the GPU tests' cases ---------------------------------------------------------------------------------
def _report(tag, dev, capsys):
    with capsys.disabled():
        print(f"\n[dpid prototype vs exact] {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in zip(NAMES, dev)), end="")


@pytest.mark.parametrize("nx", proto.NX_EDGES + (12,))      # (12: the GPU test against the device's other verbs)
def test_prototype_agrees_with_the_exact_side_at_every_group_edge(nx, capsys):
    Phi, gam, c, d, P, pro, ex = proto.edge_reference(nx)
    assert (d == 0).any() and (d > 0).any() and (P[..., 3] == 0).any() and (P[..., 3] == proto.TS / 2).any()
    dev = proto.rel_dev(pro, ex)
    _report(f"nx {nx:2d}, {proto.N_REF} x {proto.M_REF}", dev, capsys)
    assert np.isfinite(pro).all() and dev[0] <= 1e-12 and dev.max() <= 1e-10, dev


def test_prototype_agrees_on_the_bounded_cases_and_they_are_decided(capsys):
    pro, pc, ex, ec, near = proto.bounded_reference()
    dev = proto.rel_dev(pro, ex)
    _report("bounded, nx 3", dev, capsys)
    with capsys.disabled():
        print(f"; clamped ticks {ec[..., 0].min()} .. {ec[..., 0].max()}, halted {ec[..., 1].min()} .. {ec[..., 1].max()}; smallest |free - bound| "
              f"{near[..., 0].min():.2e}, smallest |e| after a clamped tick {near[..., 1].min():.2e}", end="")
    assert dev.max() <= 1e-10
    assert np.array_equal(pc, ec)
    # decided: every case, none left out
    assert near.shape == (proto.B_N, 10, 2) and (near[..., 0] >= 1e-6).all() and (near[..., 1] >= 1e-6).all()
    # and the cases exercise the law: an unclamped run is not among them, a run clamped throughout is, the integrator halts
    assert ec[..., 0].min() >= 1 and ec[..., 0].max() == N_TICKS + 1 and ec[..., 1].max() >= N_TICKS - 1 and (ec[..., 1] <= ec[..., 0]).all()


def test_infinite_bounds_and_d_zero_are_the_unbounded_arithmetic():
    """with d = 0 the bounded branch under bounds no sample reaches gives the unbounded branch's samples, to rounding: the two orders of
    summation differ by a few ulp (2.2e-16) per tick of quantities below 10, over 100 ticks: below 1e-12 in absolute terms"""
    Phi, gam, c, d, P, _, _ = proto.bounded_cases()
    args = proto.pairs(Phi, gam, c, d, P)
    B = args[4].shape[0]
    free, _, _ = proto.time_metrics(*args, np.full(B, -np.inf), np.full(B, np.inf), proto.TS, N_TICKS)
    wide, _, counts = proto.time_metrics(*args, np.full(B, -1e9), np.full(B, 1e9), proto.TS, N_TICKS)
    assert (counts == 0).all() and np.abs(wide - free).max() <= 1e-12 and np.abs(free).max() <= 10.0


def test_prototype_flags_the_failure_pairs():
    Phi, gam, c, d, P, lo, hi, expect = proto.failure_pairs()
    assert d[3] != 0.0 and d[4] == 0.0
    got, cost, st, counts = proto.metrics(*proto.pairs(Phi, gam, c, d, P), proto.W7(), proto.TS, N_TICKS, lo.reshape(-1), hi.reshape(-1))
    got, cost, st, counts = got.reshape(7, 3, 5), cost.reshape(7, 3), st.reshape(7, 3), counts.reshape(7, 3, 2)
    assert np.array_equal(st, expect), st
    assert np.isinf(got[2, 1, 1:]).all() and np.isfinite(got[2, 1, 0]) and cost[2, 1] == np.inf
    assert np.isnan(got[5, 0]).all() and cost[5, 0] == np.inf and np.isnan(got[3, 2]).all() and cost[3, 2] == np.inf and (counts[3, 2] == 0).all()
    ok = expect == 0
    assert np.isfinite(got[ok]).all() and np.isfinite(cost[ok]).all() and counts[4, 1, 0] >= 1


# ---- 3. C(z) -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [(1.3, 4.0, 0.15, 0.01), (2.0, 0.7, 0.3, 0.0), (0.5, 9.0, 0.0, 0.05)])
@pytest.mark.parametrize("theta", [0.7, 0.05, 3.0])
def test_c_of_z_is_the_laws_transfer_function(fb, p, theta, capsys):
    """the recursion driven open-loop with e_k = z^k: once the filter transient (alpha tau_f)^k has died, out_k = C(z) z^k + (the
    integrator's constant), so the quotient of successive differences is C(z)"""
    Ts = proto.TS
    kp, ki, kd, tf = p
    al = 1.0 / (tf + Ts)
    z = np.exp(1j * theta)
    xi = eta = 0.0
    out = []
    for k in range(400):
        e = z ** k
        xi = xi + Ts * ki * e
        out.append(kp * e + xi + al * (kd * e - eta))
        eta = al * tf * eta + Ts * al * kd * e
    got = (out[-1] - out[-2]) / (z ** 399 - z ** 398)
    want = kp + ki * Ts * z / (z - 1.0) + kd * al * (z - 1.0) / (z - al * tf)
    by_kernel = proto.c_response(p, Ts, np.cos(theta), np.sin(theta))
    by_wrapper = fb.dpid.dpid_response(p, Ts, np.array([theta / Ts]))[0]
    Pc, Gc, Cc, Dc = fb.build_dpid(p, Ts)
    by_model = (Cc @ np.linalg.solve(z * np.eye(2) - Pc, Gc.astype(complex)) + Dc)[0, 0]
    devs = [abs(v - want) / abs(want) for v in (got, by_kernel, by_wrapper, by_model)]
    with capsys.disabled():
        print(f"\n[C(z)] p {p}, theta {theta}: recursion {devs[0]:.1e}, the kernel's expression {devs[1]:.1e}, build_dpid {devs[3]:.1e}", end="")
    assert devs[0] <= 1e-10 and max(devs[1:]) <= 1e-13, devs


# ---- 4. the closed-loop route --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 7, 12])
def test_the_closed_loop_from_build_dpid_gives_the_laws_samples(fb, nx, capsys):
    Phi, gam, c, d = proto.dplants(nx, 4)
    P = proto.dpoints(4, 3)
    w = proto.W7()
    worst, worst_s, rho = 0.0, 0.0, 0.0
    for i in range(4):
        for j in range(3):
            y, u, _, _ = proto.law_exact(Phi[i], gam[i], c[i], d[i], P[i, j], proto.TS, N_TICKS)
            M, v, Cl, Dl = proto.closed_loop(Phi[i], gam[i], c[i], d[i], fb.build_dpid(P[i, j], proto.TS))
            rho = max(rho, np.abs(np.linalg.eigvals(M)).max())
            zk = np.zeros(M.shape[0])
            for k in range(N_TICKS + 1):
                out = Cl @ zk + Dl[:, 0]
                worst = max(worst, abs(out[0] - y[k]), abs(out[1] - u[k]), abs(out[2] - (1.0 - y[k])))
                zk = M @ zk + v[:, 0]
            for wk in w:
                zz = np.exp(1j * wk * proto.TS)
                S = (Cl[2] @ np.linalg.solve(zz * np.eye(M.shape[0]) - M, v.astype(complex)) + Dl[2])[0]
                Pz = d[i] + c[i] @ np.linalg.solve(zz * np.eye(nx) - Phi[i], gam[i].astype(complex))
                worst_s = max(worst_s, abs(S * (1.0 + Pz * fb.dpid.dpid_response(P[i, j], proto.TS, np.array([wk]))[0]) - 1.0))
    with capsys.disabled():
        print(f"\n[closed-loop route] nx {nx}: samples {worst:.1e}, S (1 + P C) - 1 {worst_s:.1e}, spectral radius <= {rho:.4f}", end="")
    assert worst <= 1e-12 and worst_s <= 1e-11 and rho < 1.0


# ---- 5. the continuous limit ------------------------------------------------------------------------------------------------------------------------------
def test_the_continuous_limit_is_first_order_in_ts(capsys):
    """the zero-order hold of one passive plant (d = 0) at Ts = 0.02, 0.005 and 0.00125 under the law, against the continuous compensator's
    metrics (pid_prototype's exact side at dt = 1.25e-4): the distance shrinks by a factor between 2 and 8 per factor 4 in Ts for ie and
    iu, and for ef and up, where the prototype shows it as well (ratios 4.0, 4.0 and 2.7, 3.6; up: u_0 = k_p + Ts k_i + k_d / (tau_f + Ts)
    against k_p + k_d / tau_f). Ms is printed and not asserted: the prototype's ratios are 4.9 and 8.4 (the peak sits at the top of the
    grid, w = 100 rad/s, where w Ts = 2 at Ts = 0.02 is far from the small-angle regime)."""
    A, b, c, d = pp.plants(3, 1)
    assert d[0] == 0.0
    p = np.array([[2.0, 6.0, 0.05, 0.05]])
    w = np.logspace(-1.0, 2.0, 25)
    cont, _, st = pp.metrics(A, b, c, d, p, w, proto.T_SIM, 1.25e-4, side="exact")
    assert (st == 0).all()
    dist = []
    for Ts in (0.02, 0.005, 0.00125):
        Phi, gam = proto.zoh(A, b, Ts)
        got, _, sd, _ = proto.metrics(Phi, gam, c, d, p, w, Ts, int(round(proto.T_SIM / Ts)))
        assert (sd == 0).all()
        dist.append(np.abs(got[0] - cont[0]))
        with capsys.disabled():
            print(f"\n[continuous limit] Ts {Ts:7.5f}: " + "  ".join(f"{k} {v:.5f} (|d| {e:.2e})" for k, v, e in zip(NAMES, got[0], dist[-1])), end="")
    with capsys.disabled():
        print("\n[continuous limit] continuous:  " + "  ".join(f"{k} {v:.5f}" for k, v in zip(NAMES, cont[0])), end="")
    dist = np.array(dist)
    for k in (1, 2, 3, 4):
        for r in (dist[0, k] / dist[1, k], dist[1, k] / dist[2, k]):
            assert 2.0 <= r <= 8.0, (NAMES[k], dist[:, k])
