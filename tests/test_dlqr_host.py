"""The discrete LQR on the device, host side (no GPU compute): fb_lss_dlqr is declared, exported, bound and wrapped; fbk::k_lss_dlqr<8 | 16>
are in the library with 0 B of scratch; the refusals that need no device; and the numpy restatement of the kernel (tests/dlqr_prototype.py)
is held to scipy.linalg.solve_discrete_are and to the Riccati residual on exactly the GPU test's cases (tests/test_gpu_dlqr.py), which are
checked to be fair: scipy's own residual <= 1e-11, the closed loop of scipy's K inside the unit circle, the prototype's status 0.

What the prototype is held to (none of it taken from what the prototype gives):
  the residual   no worse than the yardstick's own on the same systems (floor 1e-13: the fp64 level of sums of <= 16 terms over <= 16 doublings);
  X              a residual E of the Riccati equation moves its solution by inv(T) E to first order, T: dX -> dX - Phic' dX Phic the closed
                 loop's Stein operator, |inv(T)|_2 <= sum_k |Phic^k|_2^2 =: s. With nx for the change between the largest entry and the
                 2-norm, twice, and 2 for what first order leaves out and for the rounding of the residuals' own evaluation (in the scalar
                 case the first-order statement is an equality): max|X - X_scipy| <= 2 nx^2 s (E_prototype + E_scipy), absolute residuals;
  K              the gain comes out of the closed loop, K = inv(R) Gam' X inv(I + G0 X) Phi; the textbook form solves (R + Gam' X Gam) K =
                 Gam' X Phi. At the prototype's own X the two differ by rounding: 64 nx cond(R + Gam' X Gam) cond(I + G0 X) 2^-52 of max|K|.
  the doublings  the GPU test asks for the prototype's count on every system. Another rounding of the same arithmetic counts the same unless a
                 deciding quantity sits within rounding of its threshold: max|dH| is a difference of entries of H, so one unit in the last
                 place of H moves max|dH| / (1e-13 max|H|) by 2^-52 / 1e-13 = 2.2e-3; max|A| against 2^-20 moves by rounding only. Asked
                 here: every deciding quantity of every doubling at least a factor 1.01 from its threshold, on either side.
The deviations from scipy are printed: the GPU test's bounds are ten times them, computed there over the same systems."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import c2d_prototype as c2d
import dlqr_prototype as proto
import lqr_prototype as lq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_HOST = proto.N_DISTINCT          # the distinct systems of a GPU case (tests/dlqr_prototype.py, batch)
EPS = 2.0 ** -52


def test_the_symbol_is_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    assert "fb_lss_dlqr" in declared and re.search(r"\bT fb_lss_dlqr\b", out)
    assert "fb_lss_dlqr" in fb.EXPORTED and len(fb.lib.fb_lss_dlqr.argtypes) == 9
    assert "(:fb_lss_dlqr, lib)" in shim and re.search(r"^function dlqr\(w::LinearWorld", shim, flags=re.M)
    want = (1, 2, 40, 16)
    assert tuple(fb.K[k] for k in ("FB_DLQR_NOT_CONVERGED", "FB_DLQR_SINGULAR", "FB_DLQR_MAX_ITERS", "FB_DLQR_NX_MAX")) == want
    assert (proto.NOT_CONVERGED, proto.SINGULAR, proto.MAX_ITERS, proto.NX_MAX) == want
    assert callable(fb.dlqr) and hasattr(fb, "DlqrResult") and fb.dlqr is fb.lqr.__globals__["dlqr"]
    import inspect
    assert list(inspect.signature(fb.dlqr).parameters) == ["world", "Q", "R", "closed"] and inspect.signature(fb.dlqr).parameters["closed"].default is False
    assert {"K", "X", "resid", "iters", "status", "world"} <= set(fb.DlqrResult.__dataclass_fields__) and isinstance(fb.DlqrResult.success, property)


def test_the_kernels_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    # per group two P x (P + 2) panels, the solve's rows P x 2 P and its pivot row 3 P
    want = {f"fbk::k_lss_dlqr<{P}>": (2 * P * (P + 2) + 2 * P * P + 3 * P) * (64 // P) * 8 for P in (8, 16)}
    assert {k for k in ks if k.startswith("fbk::")} == set(want), sorted(k for k in ks if k.startswith("fbk::"))
    for name, lds in want.items():
        print(name, ks[name])
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == lds and ks[name]["vgpr"] <= 512, (name, ks[name])


def test_refusals_that_need_no_device(fb):
    h = C.c_void_p(1)
    assert fb.lib.fb_lss_dlqr(None, None, None, None, None, None, None, None, C.byref(h)) != 0 and b"null handle" in fb.lib.fb_last_error() and not h.value
    assert fb.lib.fb_lss_dlqr(None, None, None, None, None, None, None, None, None) != 0 and b"null handle" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError, match="LinearWorld"):
        fb.dlqr(object(), np.eye(2), np.eye(1))


# ---- the prototype against scipy over the GPU test's cases, and the cases themselves -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(nx, nu, Ts):
    A, B, Phi, Gam, Q, R = proto.sampled(nx, nu, N_HOST, Ts)
    return Phi, Gam, Q, R, proto.designs(Phi, Gam, Q, R)


@pytest.mark.parametrize("Ts", proto.TS_ALL)
@pytest.mark.parametrize("nx,nu", proto.SHAPES)
def test_prototype_against_scipy_on_fair_cases(nx, nu, Ts, capsys):
    Phi, Gam, Q, R, (got, Ks, Xs) = _case(nx, nu, Ts)
    n = Phi.shape[0]
    assert (got["status"] == 0).all()
    rs = np.array([proto.residual(Phi[i], Gam[i], Q, Ks[i], Xs[i]) for i in range(n)])
    radius = np.array([proto.rho(Phi[i] - Gam[i] @ Ks[i]) for i in range(n)])
    assert rs.max() <= 1e-11 and radius.max() < 1.0                                                   # the case is fair
    rp = np.array([proto.residual(Phi[i], Gam[i], Q, got["K"][i], got["X"][i]) for i in range(n)])    # the contract's form, by the host's products
    dK, dX = proto.rel_dev(got["K"], Ks), proto.rel_dev(got["X"], Xs)
    with capsys.disabled():
        print(f"\n[dlqr prototype vs scipy] ({nx:2d}, {nu}) Ts {Ts:g} x {n}: K {dK:.2e}  X {dX:.2e}  resid <= {got['resid'].max():.2e} (the contract's form "
              f"{rp.max():.2e}; scipy's own {rs.max():.2e})  doublings {got['iters'].min()} - {got['iters'].max()} (every decision a factor >= {got['margin'].min():.3f} from its threshold)  rho <= {radius.max():.4f}", end="")
    assert 1 <= got["iters"].min() and got["iters"].max() <= 20 and got["margin"].min() >= proto.DECISION_MIN
    assert max(got["resid"].max(), rp.max()) <= max(rs.max(), proto.RESID_FLOOR)
    assert np.array_equal(got["X"], got["X"].transpose(0, 2, 1))
    for i in range(n):
        scale = max(np.abs(Q).max(), np.abs(Xs[i]).max())
        bound = 2 * nx * nx * proto.sensitivity(Phi[i], Gam[i], Ks[i]) * (rp[i] + rs[i]) * scale
        assert np.abs(got["X"][i] - Xs[i]).max() <= bound, (i, np.abs(got["X"][i] - Xs[i]).max(), bound)
        X = got["X"][i]
        M = R + Gam[i].T @ X @ Gam[i]
        Kt = np.linalg.solve(M, Gam[i].T @ X @ Phi[i])
        W = np.eye(nx) + Gam[i] @ np.linalg.solve(R, Gam[i].T) @ X
        tol = 64 * nx * np.linalg.cond(M) * np.linalg.cond(W) * EPS
        assert np.abs(got["K"][i] - Kt).max() <= tol * np.abs(Kt).max(), (i, np.abs(got["K"][i] - Kt).max() / np.abs(Kt).max(), tol)


def test_the_three_systems_without_a_solution(capsys):
    """on their own weights at Ts = 0.25, and as the GPU test embeds them (one pair of weights for the batch)"""
    own = []
    for a, b, q, r, _ in lq.failure_systems():
        Ph, Ga, _, _, st = c2d.c2d(a, b, np.zeros(a.shape[0]), 0.25)
        assert st == 0
        o = proto.dlqr(Ph, Ga, q, r)
        own.append((o["status"], o["iters"]))
        assert np.isnan(o["K"]).all() and np.isnan(o["X"]).all() and np.isnan(o["resid"])
    A, B, Q, R, where, want = proto.failure_case()
    Phi, Gam, _, _, st = c2d.c2d_batch(A, B, np.zeros((A.shape[0], 3)), 0.25)
    emb = [proto.dlqr(Phi[i], Gam[i], Q, R) for i in where]
    with capsys.disabled():
        print(f"\n[dlqr prototype, no stabilising solution] (status, doublings) own weights {own}; embedded {[(o['status'], o['iters']) for o in emb]}", end="")
    assert [s for s, _ in own] == [proto.SINGULAR, proto.NOT_CONVERGED, proto.NOT_CONVERGED] == [o["status"] for o in emb] == list(want)
    assert own[1][1] == own[2][1] == proto.MAX_ITERS and own[0][1] < proto.MAX_ITERS
    healthy = [i for i in range(A.shape[0]) if i not in where]
    assert all(proto.dlqr(Phi[i], Gam[i], Q, R)["status"] == 0 for i in healthy)
    # a NaN in A: Phi is NaN after c2d, the first solve finds no pivot
    bad = np.full((3, 3), np.nan)
    o = proto.dlqr(bad, Gam[0], Q, R)
    assert (o["status"], o["iters"]) == (proto.SINGULAR, 1)


def test_the_integrator_chain_and_a_singular_phi(capsys):
    one = lambda v: np.array(v, dtype=np.float64)
    Ph, Ga, _, _, _ = c2d.c2d(one([[0, 1], [0, -2]]), one([[0], [1]]), np.zeros(2), 0.02)
    o = proto.dlqr(Ph, Ga, np.eye(2), np.eye(1))
    Ks, Xs = proto.scipy_dlqr(Ph, Ga, np.eye(2), np.eye(1))
    # Phi with an eigenvalue at 0 (a pure delay): nothing inverts Phi
    Pd, Gd = one([[0, 1], [0, 0]]), one([[0], [1]])
    od = proto.dlqr(Pd, Gd, np.eye(2), np.eye(1))
    Kd, Xd = proto.scipy_dlqr(Pd, Gd, np.eye(2), np.eye(1))
    with capsys.disabled():
        print(f"\n[dlqr prototype] integrator chain at Ts 0.02: {o['iters']} doublings, resid {o['resid']:.2e}, X vs scipy "
              f"{np.abs(o['X'] - Xs).max() / np.abs(Xs).max():.2e}; a delay (Phi singular): {od['iters']} doublings, resid {od['resid']:.2e}", end="")
    assert o["status"] == 0 and od["status"] == 0
    assert o["resid"] <= max(proto.residual(Ph, Ga, np.eye(2), Ks, Xs), proto.RESID_FLOOR)
    assert np.abs(od["X"] - Xd).max() <= 16 * EPS * np.abs(Xd).max() and np.abs(od["K"] - Kd).max() <= 16 * EPS          # (two doublings end it: A = 0 exactly)


# ---- the cases of the GPU test's cost identity and continuous limit: how long they step, how far apart the two designs are ------------------------------
@pytest.mark.parametrize("nx,nu", proto.COST_SHAPES)
def test_the_cost_identity_on_the_prototypes_own_map(nx, nu, capsys):
    A, B, Phi, Gam, Q, R = proto.sampled(nx, nu, proto.COST_N, proto.COST_TS)
    got, Ks, Xs = proto.designs(Phi, Gam, Q, R)
    radius = max(proto.rho(Phi[i] - Gam[i] @ Ks[i]) for i in range(proto.COST_N))
    M = int(np.ceil(17.0 / -np.log(radius)))
    dx0 = np.random.default_rng(nx).standard_normal((proto.COST_N, nx))
    J, want, end = proto.cost(Phi, Gam, Q, R, got["K"], got["X"], dx0, M)
    q = np.abs(J - want) / want
    with capsys.disabled():
        print(f"\n[dlqr prototype, optimal cost] ({nx:2d}, {nu}) Ts {proto.COST_TS}: rho <= {radius:.4f}, M {M}: |sum - dx0' X dx0| / (dx0' X dx0) <= {q.max():.2e}; "
              f"|dx_M| / |dx0| <= {end.max():.2e}", end="")
    assert radius <= 0.992 and M < 2200
    # the tail past M is below rho^(2 M) <= e^-34 of the cost; what is left is the rounding of M sums and of X itself (the bound on X above)
    assert q.max() <= 1e-9 and end.max() <= 1e-4


def test_the_continuous_limit_by_scipy(capsys):
    from scipy.linalg import solve_continuous_are
    A, B, Q, R = lq.systems(5, 2, 3)
    Kc = np.array([np.linalg.solve(R, B[i].T @ solve_continuous_are(A[i], B[i], Q, R)) for i in range(3)])
    d = []
    for Ts in proto.LIMIT_TS:
        Phi, Gam = c2d.exact_batch(A, B, np.zeros((3, 5)), Ts)[:2]
        Kd = proto.scipy_batch(Phi, Gam, Ts * Q, Ts * R)[0]
        d.append(proto.rel_dev(Kd, Kc))
    with capsys.disabled():
        print(f"\n[dlqr, the continuous limit by scipy] (5, 2) x 3: |K_d(Ts Q, Ts R) - K_c| / max|K_c| at Ts {proto.LIMIT_TS}: " + ", ".join(f"{v:.2e}" for v in d), end="")
    assert 2e-2 <= d[0] <= 4e-2 and all(1.7 <= d[k] / d[k + 1] <= 2.3 for k in range(2))          # first order in Ts
