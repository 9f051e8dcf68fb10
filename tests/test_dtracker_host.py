"""Discrete LQR trackers on the device, host side (no GPU compute; docs/design/linearize.md, "Discrete LQR trackers on the device"):

  1. fb_lss_dtracker_metrics and fb_lss_dsteady are declared, exported, bound and wrapped, and refuse a NULL handle by name; the kernels of
     namespace fbj are exactly the three instances of k_dtracker and of k_dsteady, each with 0 B of scratch, k_dtracker with the one
     exchange panel (512 B) of LDS; header, kernel and prototype agree on the constants; the wrapper's refusals that need no device;
  2. the numpy restatement of the kernel (tests/dtracker_prototype.py) is held to the exact side (a literal tick-by-tick transcription of
     the law) on every case tests/test_gpu_dtracker.py uses: stable and unstable Phi, nx + nu + nz at every group edge, D_z = 0 and != 0 —
     the deviations printed here are what the GPU bound multiplies;
  3. the conversion identity: the design-form loop u_k = -K_x x_k - K_xi xi_k-1 + (K_fwd + Ts K_xi) zref equals the flown form with
     K_int = K_xi, K_fbk = K_x - Ts K_xi C_z;
  4. the discrete steady-state map against numpy.linalg.solve: Phi X + Gamma U = X, C_z X + D_z U = I, and the unbounded flown law with an
     integrator settles on zref;
  5. every bounded case is decided: no free_k within 1e-6 (over max(1, |bound|)) of a bound and no integrator input within 1e-6 of zero
     after a clamped tick, so rounding cannot change the clamp or halt history and the device's counts must equal the exact side's integers.

Bounds. Prototype against the exact side: the two differ in summation order only (ascending column loops against matrix-vector products);
over 100 ticks of maps with spectral radius up to 1.02 and nx <= 16 that is a few hundred ulp of the largest sample of a response, and
ef = |zref - z_N|, a difference of two numbers of order one, sees it 1 / ef times larger: asserted at 1e-12 on the samples and 1e-10 on the
metrics."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dtracker_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fb_lss_dtracker_metrics", "fb_lss_dsteady")
D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
pd = lambda a: a.ctypes.data_as(D)
pi = lambda a: a.ctypes.data_as(I)


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_bound_and_wrapped(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h"), encoding="utf-8").read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name, nargs in zip(NAMES, (17, 12)):
        assert name in declared and re.search(rf"\bT {name}\b", out)
        assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == nargs
        assert f"(:{name}, lib)" in shim
    assert set(fb.EXPORTED) == declared
    assert list(inspect.signature(fb.dsteady_state).parameters) == ["world", "z", "K", "K_xi"]
    assert list(inspect.signature(fb.dtracker_metrics).parameters)[:9] == ["world", "z", "K_fbk", "K_fwd", "K_int", "zref", "t_sim", "bounds", "stride"]
    assert list(inspect.signature(fb.dlqr_tracker).parameters)[:6] == ["world", "z", "Q", "R", "Q_int", "forward"]
    assert list(inspect.signature(fb.dtracker_world).parameters)[:5] == ["world", "z", "K_fbk", "K_fwd", "K_int"]
    assert list(inspect.signature(fb.dintegrators_world).parameters)[:3] == ["n", "k", "Ts"]
    assert list(inspect.signature(fb.dintegral_augmentation).parameters)[:2] == ["world", "z"]


def test_both_verbs_refuse_a_null_handle_by_name(fb):
    iz, g, zr, st = np.zeros(1, dtype=np.int32), np.ones(1), np.ones(1), np.empty(1, dtype=np.int32)
    rc = fb.lib.fb_lss_dtracker_metrics(None, pi(iz), 1, pd(g), pd(g), pd(g), None, 1, pd(zr), 2.0, 1, None, None, None, None, None, pi(st))
    err = fb.lib.fb_last_error()
    assert rc != 0 and b"null handle" in err and b"fb_lss_dtracker_metrics" in err, err
    rc = fb.lib.fb_lss_dsteady(None, pi(iz), 1, None, None, 0, None, None, None, None, None, pi(st))
    err = fb.lib.fb_last_error()
    assert rc != 0 and b"null handle" in err and b"fb_lss_dsteady" in err, err


def test_the_constants_agree(fb):
    assert tuple(fb.K[k] for k in ("FB_DTRACK_DIVERGED", "FB_DTRACK_NOT_FINITE", "FB_DTRACK_ROWS_MAX", "FB_DSTEADY_DIRECT")) == (
        proto.DIVERGED, proto.NOT_FINITE, proto.ROWS_MAX, proto.DIRECT) == (1, 2, 32, 4)
    assert (fb.dtracker.DIVERGED, fb.dtracker.NOT_FINITE, fb.dtracker.ROWS_MAX, fb.dtracker.DIRECT) == (1, 2, 32, 4)
    assert fb.K["FB_DSTEADY_DIRECT"] & (fb.K["FB_SURGERY_SINGULAR"] | fb.K["FB_SURGERY_NOT_FINITE"]) == 0
    text = open(os.path.join(ROOT, "flight.jl_amd", "csrc", "dtracker_kernels.hpp"), encoding="utf-8").read()
    assert float(re.search(r"constexpr double DTRACK_BLOWUP = ([0-9.e+]+);", text).group(1)) == proto.BLOWUP
    assert "#pragma unroll 1\n    for (int k = 0; k <= N; k++)" in text      # the tick loop is not unrolled
    assert max(sum(v) for v in proto.EDGES.values()) == proto.ROWS_MAX and all(sum(v) == k for k, v in proto.EDGES.items())


def test_the_kernel_instances_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    want = {f"fbj::k_{verb}<{P}>" for verb in ("dtracker", "dsteady") for P in (8, 16, 32)}
    assert {k for k in ks if k.startswith("fbj::")} == want, sorted(k for k in ks if k.startswith("fbj::"))
    for name in sorted(want):
        print(name, ks[name])
        assert ks[name]["scratch"] == 0
        if "dtracker" in name:
            assert ks[name]["lds"] == 64 * 8                        # one double per lane: the exchange panel
    for P in (8, 16, 32):                                           # the continuous map keeps its name, and its LDS is the discrete one's
        assert ks[f"fbm::k_steady<{P}>"]["lds"] == ks[f"fbj::k_dsteady<{P}>"]["lds"]


class _World:
    n, nx, nu, ny = 3, 2, 1, 2
    x_labels, u_labels, y_labels = ("a", "b"), ("u",), ("y", "a")
    _h = None
    Ts = 0.02


def test_wrapper_refusals_that_need_no_device(fb):
    w = _World()
    with pytest.raises(fb.FlightBatchError, match="LinearWorld"):
        fb.dtracker_metrics(w, ["y"], np.ones((1, 2)), np.ones((1, 1)), np.ones((1, 1)), 1.0, 2.0)
    with pytest.raises(fb.FlightBatchError, match="LinearWorld"):
        fb.dsteady_state(w, ["y"])
    from flightbatch.dtracker import _pair_gain, _pack_pairs, _u_bounds
    for bad in (np.ones((2, 2)), np.ones((2, 1, 2)), np.ones((3, 2, 1, 3))):
        with pytest.raises(ValueError, match="K_fbk must be"):
            _pair_gain(bad, 3, 2, 1, 2, "K_fbk")
    g = _pair_gain(np.arange(12.0).reshape(3, 2, 1, 2), 3, 2, 1, 2, "K_fbk")
    flat = _pack_pairs(g)                                           # element (r, c) of pair (i, j) at [((r + rows c) m + j) N + i]
    assert flat[((0 + 1 * 1) * 2 + 1) * 3 + 2] == g[2, 1, 0, 1]
    for bnd in ((1.0, 1.0), (2.0, -2.0), (np.nan, 1.0), (-1.0, np.nan), (np.inf, np.inf), (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match="bounds"):
            _u_bounds(bnd, 3, 2, 1, None)
    b = _u_bounds((np.array([-1.0, -2.0]), 3.0), 3, 4, 2, np.array([0.5, 1.0]))       # absolute bounds: u_trim is subtracted
    assert b.shape == (2 * 2 * 4 * 3,) and b[0] == -1.5 and b[4 * 3] == -3.0 and b[2 * 4 * 3] == 2.5 and b[3 * 4 * 3] == 2.0


# ---- 2. the prototype against the exact side on the GPU tests' cases ---------------------------------------------------------------------------------
def _report(tag, dev, capsys):
    with capsys.disabled():
        print(f"\n[dtracker prototype vs exact] {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in dev.items()), end="")


def _held(dev):
    return dev["zs"] <= 1e-12 and dev["us"] <= 1e-12 and dev["zmet"] <= 1e-10 and dev["umet"] <= 1e-10


@pytest.mark.parametrize("rows,n,m", [(r, proto.N_REF, proto.M_REF) for r in proto.EDGES] + list(proto.BIG))
def test_prototype_agrees_with_the_exact_side_at_every_group_edge(rows, n, m, capsys):
    Phi, _, _, Dz, _, _, _, _, pro, ex = proto.edge_reference(rows, n, m)
    rho = np.abs(np.linalg.eigvals(Phi)).max(axis=1)
    assert n < 4 or ((rho > 1.0).any() and (rho < 1.0).any())
    assert (Dz[0::2] == 0).all() and (Dz[1::2] != 0).any()
    dev = proto.deviations(pro, ex)
    _report(f"rows {rows:2d} (nx, nu, nz = {proto.EDGES[rows]}), {n} x {m}", dev, capsys)
    assert all(np.isfinite(pro[k]).all() for k in proto.KEYS) and _held(dev), dev
    assert (pro["counts"] == 0).all() and (ex["counts"] == 0).all()


def test_prototype_agrees_on_the_bounded_cases_and_they_are_decided(capsys):
    pro, ex, near = proto.bounded_reference()
    lo, hi = proto.bounded_cases()[7:]
    n, m = lo.shape[:2]
    dev = proto.deviations(pro, ex)
    _report("bounded, nx 3, nu 2, nz 2", dev, capsys)
    ec = ex["counts"].reshape(n, m, 2, 2)
    with capsys.disabled():
        print(f"; clamped ticks up to {ec[..., 0].max()}, halted up to {ec[..., 1].max()}; smallest |free - bound| / max(1, |bound|) "
              f"{near[:, 0].min():.2e}, smallest |K_int e| after a clamped tick {near[:, 1].min():.2e}", end="")
    assert _held(dev), dev
    assert np.array_equal(pro["counts"], ex["counts"])
    # decided: every pair, none left out
    assert near.shape == (n * m, 2) and (near >= 1e-6).all(), near.min(axis=0)
    # and the cases exercise the law: halted ticks, a pair that clamps on one input only, both inputs clamped, bounds never reached
    assert ec[..., 1].max() > 0 and (ec[..., 1] <= ec[..., 0]).all()
    assert ((ec[:, :, 0, 0] > 0) & (ec[:, :, 1, 0] == 0)).any() and ((ec[:, :, 0, 0] == 0) & (ec[:, :, 1, 0] > 0)).any()
    assert (ec[:, :, :, 0] > 0).all(axis=2).any() and (ec[:, 4] == 0).all() and (ec[:, 5] == 0).all()
    # infinite bounds are no bounds: the same numbers
    un = proto.tracker(*proto.pairs(*proto.bounded_cases()[:7]), proto.B_ZREF, proto.TS, proto.N_TICKS)
    for k in proto.KEYS:
        assert np.array_equal(un[k].reshape((n, m) + un[k].shape[1:])[:, 5], pro[k].reshape((n, m) + pro[k].shape[1:])[:, 5]), k


def test_prototype_flags_the_failure_pairs():
    Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, expect = proto.failure_pairs()
    zref = proto.plants(2, 1, 1, 6)[4]
    res = proto.tracker(*proto.pairs(Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint), zref, proto.TS, proto.N_TICKS)
    assert np.array_equal(res["status"].reshape(expect.shape), expect)
    zm = res["zmet"].reshape(expect.shape + (1, 3))
    assert np.isinf(zm[2, 1]).all() and np.isnan(zm[4, 0]).all() and np.isnan(zm[4, 2]).all() and np.isfinite(zm[expect == 0]).all()


def test_sample_rows_follow_the_family_rule():
    assert proto.sample_rows(100, 1).tolist() == list(range(101))
    assert proto.sample_rows(100, 7).tolist() == list(range(0, 100, 7)) + [100] and len(proto.sample_rows(100, 7)) == 16      # ceil(100 / 7) + 1
    assert proto.sample_rows(100, 10).tolist() == list(range(0, 101, 10)) and proto.sample_rows(100, 100).tolist() == [0, 100]


# ---- 3. the conversion identity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [8, 15])
def test_design_form_equals_flown_form(rows, capsys):
    nx, nu, nz = proto.EDGES[rows]
    Phi, Gam, Cz, _, zref = proto.plants(nx, nu, nz, 8)
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in range(0, 8, 2):                                        # (D_z = 0 on the even systems)
        K_aug = np.concatenate([0.05 * rng.standard_normal((nu, nx)), 0.5 * rng.standard_normal((nu, nz))], axis=1)
        K_fwd = rng.standard_normal((nu, nz))
        K_x, K_xi = K_aug[:, :nx], K_aug[:, nx:]
        zd, ud = proto.design_form(Phi[k], Gam[k], Cz[k], K_aug, K_fwd, zref, proto.TS, proto.N_TICKS)
        zf, uf, _, _ = proto.law_exact(Phi[k], Gam[k], Cz[k], np.zeros((nz, nu)), K_x - proto.TS * K_xi @ Cz[k], K_fwd, K_xi, zref, proto.TS, proto.N_TICKS)
        worst = max(worst, np.abs(zd - zf).max() / np.abs(zf).max(), np.abs(ud - uf).max() / np.abs(uf).max())
    with capsys.disabled():
        print(f"\n[design form vs flown form, rows {rows}] worst deviation over the largest sample {worst:.2e}", end="")
    assert worst <= 1e-12          # the same loop written two ways: rounding only


# ---- 4. the discrete steady-state map --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(1, 1), (7, 2), (14, 3), (24, 8)])       # nx + nu = 2, 9, 17, 32
def test_dsteady_is_the_equilibrium_of_the_map(nx, nu):
    Phi, Gam, Cz, Dz, _ = proto.plants(nx, nu, nu, 6)
    rng = np.random.default_rng(4)
    for k in range(6):
        K, K_xi = rng.standard_normal((nu, nx)), rng.standard_normal((nu, nu))
        X, U, K_fbk, K_fwd = proto.dsteady(Phi[k], Gam[k], Cz[k], Dz[k], K, K_xi)
        assert np.abs(Phi[k] @ X + Gam[k] @ U - X).max() <= 1e-10 * max(1.0, np.abs(X).max())
        assert np.abs(Cz[k] @ X + Dz[k] @ U - np.eye(nu)).max() <= 1e-10 * max(1.0, np.abs(X).max(), np.abs(U).max())
        assert np.array_equal(K_fbk, K - proto.TS * K_xi @ Cz[k]) and np.array_equal(K_fwd, U + K_fbk @ X)


def test_the_flown_law_with_an_integrator_settles_on_zref():
    Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, _, _ = proto.bounded_cases()
    zs, us, _, _ = proto.law_exact(Phi[0], Gam[0], Cz[0], Dz[0], Kfbk[0, 0], Kfwd[0, 0], Kint[0, 0], proto.B_ZREF, proto.TS, 3000)
    assert np.abs(zs[:, -1] - proto.B_ZREF).max() <= 1e-9
    X, U, _, _ = proto.dsteady(Phi[0], Gam[0], Cz[0], Dz[0])
    assert np.abs(us[:, -1] - U @ proto.B_ZREF).max() <= 1e-8          # the inputs that hold it are the map's U zref
