"""Closing loops on the device, host side (no GPU compute): fb_lss_connect and fb_lss_get_cd are declared, exported, bound and wrapped;
fbc::k_connect<8 | 16 | 32> are in the library with 0 B of scratch; the refusals that need no device; the numpy restatement of the kernel
(tests/connect_prototype.py) reproduces the host surgery of the tree — the notebook's two loops, the q2e plant and flightbatch.lqr.closed_loop
exactly, pid_prototype.closed_loop within 4 ulp of each matrix's largest entry — and on the generator of the GPU tests its float64 side stays
within 1e-14 of its longdouble side, the condition under which tests/test_gpu_connect.py's accuracy rule means what it says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import connect_prototype as proto
import pid_prototype
import timeresp_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_the_symbols_are_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name, nargs in (("fb_lss_connect", 13), ("fb_lss_get_cd", 3)):
        assert name in declared
        assert re.search(r"\bT %s\b" % name, out)
        assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == nargs
        assert f"(:{name}, lib)" in shim
    assert re.search(r"^function connect\(p::LinearWorld", shim, flags=re.M) and re.search(r"^function model_cd\(w::LinearWorld", shim, flags=re.M)
    K = fb.K
    assert (K["FB_CONNECT_ILL_POSED"], K["FB_CONNECT_NOT_FINITE"], K["FB_CONNECT_NV_MAX"], K["FB_CONNECT_NF_MAX"], K["FB_CONNECT_NZ_MAX"]) == (1, 2, 16, 32, 128)
    assert (proto.ILL_POSED, proto.NOT_FINITE, proto.NV_MAX, proto.NF_MAX, proto.NZ_MAX) == (1, 2, 16, 32, 128)
    import importlib
    cn = importlib.import_module("flightbatch.connect")      # (the package attribute of that name is the verb)
    assert (cn.ILL_POSED, cn.NOT_FINITE, cn.NV_MAX, cn.NF_MAX, cn.NZ_MAX) == (1, 2, 16, 32, 128)
    for name in ("connect", "ConnectResult", "integrator_world", "pid_world", "state_feedback", "unity_feedback"):
        assert hasattr(fb, name) and getattr(fb, name) is getattr(cn, name)
    assert callable(fb.LinearWorld.model_cd) and callable(fb.LinearWorld.model)


def test_the_kernels_are_in_the_library(tmp_path_factory):
    """exactly the instances the dispatcher of fb_lss_connect can launch (csrc/fb_lss.inc: family_launch, group_for), with the resources the doc tabulates"""
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    lds = {"fbc::k_connect<8>": 10240, "fbc::k_connect<16>": 14080, "fbc::k_connect<32>": 11392}
    assert {k for k in ks if k.startswith("fbc::")} == set(lds), sorted(k for k in ks if k.startswith("fbc::"))
    for name, want in lds.items():
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == want, (name, ks[name])
        assert not re.search(r"\bk_step_", name) and "k_lss_" not in name and "k_lqr" not in name
    assert {proto.group(s[0] + s[1], s[2] + s[3]) for s in proto.SHAPES} == {8, 16, 32}


def test_refusals_that_need_no_device(fb):
    h = C.c_void_p(1)
    one = np.zeros(1, dtype=np.int32)
    g = np.ones(1)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = fb.lib.fb_lss_connect(None, None, pi(one), 1, pd(g), 0, pd(g), 0, 1, None, 0, None, C.byref(h))
    assert rc != 0 and b"fb_lss_connect" in fb.lib.fb_last_error() and b"null handle" in fb.lib.fb_last_error() and not h.value
    rc = fb.lib.fb_lss_connect(None, None, pi(one), 1, pd(g), 0, pd(g), 0, 1, None, 0, None, None)
    assert rc != 0 and b"out is null" in fb.lib.fb_last_error()
    assert fb.lib.fb_lss_get_cd(None, None, None) != 0 and b"null handle" in fb.lib.fb_last_error()


# ---- the host surgery of the tree ----------------------------------------------------------------------------------------------------------------
def _robot2d():
    import json
    lin = json.load(open(os.path.join(timeresp_prototype.GOLDEN, "robot2d_linearization.json"), encoding="utf-8"))
    return tuple(np.array(lin[k]) for k in "ABCD")


def notebook_wiring():
    """(jz, F, G) of the velocity loop around Robot2D (z = ω, v, θ, η, u_m, τ_m, ξ; v = m, ξ'): m = K_fwd v_ref - K_x (ω, v, θ) - ξ,
    ξ' = K_int (v - v_ref); and of the position loop around that: v_ref = 0.6 (η_ref - η)"""
    from support import gains_from_h5
    g = gains_from_h5()
    K_x, K_fwd, K_int = g[0:3], g[3], g[4]
    F = np.array([[-K_x[0], -K_x[1], -K_x[2], -1.0], [0.0, K_int, 0.0, 0.0]])
    G = np.array([[K_fwd], [-K_int]])
    return ([0, 1, 2, 6], F, G), ([3], np.array([[-0.6]]), np.array([[0.6]]))


def test_prototype_reproduces_the_notebooks_loops_exactly():
    (Av, bv, cv, dv), (Ap, bp, ce, dp) = timeresp_prototype.notebook_loops_from_golden()
    vel, pos = notebook_wiring()
    A1, B1, C1, D1, st = proto.connect(_robot2d(), proto.integrator(), *vel, None)
    assert st == 0 and C1.shape == (7, 5) and D1.shape == (7, 1)
    assert np.array_equal(A1, Av) and np.array_equal(B1[:, 0], bv) and np.array_equal(C1[1], cv) and D1[1, 0] == dv
    A2, B2, C2, D2, st = proto.connect((A1, B1, C1, D1), None, *pos, None)
    assert st == 0 and np.array_equal(A2, Ap) and np.array_equal(B2[:, 0], bp) and np.array_equal(C2[3], ce) and D2[3, 0] == dp
    # the longdouble side on the same inputs is the float64 side (every added term is an exact zero, every product of two doubles the same)
    L = proto.connect(_robot2d(), proto.integrator(), *vel, None, dtype=np.longdouble)
    assert L[0].dtype == np.longdouble and np.array_equal(L[0].astype(np.float64), A1)


def q2e_wiring(K_fbk, K_fwd, i_ele=1):
    """(jz, F, G) of pid_prototype.q2e_plant: the te2te design model (C = I, 8 outputs) with the integrator behind it; u = K_fwd[:, elevator] ξ
    - K_fbk x, the integrator's input is w"""
    nu, nx = K_fbk.shape
    F = np.zeros((nu + 1, nx + 1))
    F[:nu, :nx] = -K_fbk
    F[:nu, nx] = K_fwd[:, i_ele]
    G = np.zeros((nu + 1, 1)); G[nu, 0] = 1.0
    return list(range(nx + 1)), F, G


def test_prototype_reproduces_the_q2e_plant_exactly():
    rng = np.random.default_rng(3)
    for _ in range(20):
        A, B, K_fbk, K_fwd = rng.standard_normal((8, 8)), rng.standard_normal((8, 2)), rng.standard_normal((2, 8)), rng.standard_normal((2, 2))
        A9, b9, c9, d9 = pid_prototype.q2e_plant(A, B, K_fbk, K_fwd)
        plant = (A, B, np.eye(8), np.zeros((8, 2)))
        A1, B1, C1, D1, st = proto.connect(plant, proto.integrator(), *q2e_wiring(K_fbk, K_fwd), [0])
        assert st == 0 and np.array_equal(A1, A9) and np.array_equal(B1[:, 0], b9) and np.array_equal(C1[0], c9) and D1[0, 0] == d9


def test_prototype_reproduces_closed_loop_exactly(fb):
    rng = np.random.default_rng(4)
    n, nx, nu = 5, 6, 3
    m = fb.design_model(rng.standard_normal((n, nx, nx)), rng.standard_normal((n, nx, nu)))
    K = rng.standard_normal((n, nu, nx))
    cl = fb.closed_loop(m, K)
    got = proto.connect_batch((m.A, m.B, m.C, m.D), None, list(range(nx)), -K, np.eye(nu), None)
    assert (got[4] == 0).all()
    for a, b in zip(got[:4], (cl.A, cl.B, cl.C, cl.D)):
        assert np.array_equal(a, b)
    # and with a direct term: C - D K
    m.D[:] = rng.standard_normal(m.D.shape)
    m.C[:] = rng.standard_normal(m.C.shape)
    cl = fb.closed_loop(m, K)
    # (C is no longer I: the loop closed on the states needs them as outputs, so the identity rows go in front)
    C2 = np.concatenate([np.broadcast_to(np.eye(nx), (n, nx, nx)), m.C], axis=1)
    D2 = np.concatenate([np.zeros((n, nx, nu)), m.D], axis=1)
    got = proto.connect_batch((m.A, m.B, C2, D2), None, list(range(nx)), -K, np.eye(nu), list(range(nx, 2 * nx)))
    for a, b in zip(got[:4], (cl.A, cl.B, cl.C, cl.D)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("nx", [1, 5, 8])
def test_prototype_reproduces_the_pid_loop_within_4_ulp(nx, capsys):
    n = 40
    A, b, c, d = pid_prototype.plants(nx, n)
    P = pid_prototype.points(n, 1)[:, 0]
    worst = np.zeros(6)
    for k in range(n):
        M, c0, (yrow, yc), (urow, uc) = pid_prototype.closed_loop(A[k], b[k], c[k], d[k], P[k])
        plant = (A[k], b[k][:, None], c[k][None, :], np.array([[d[k]]]))
        A1, B1, C1, D1, st = proto.unity_feedback(plant, proto.pid(P[k]))
        assert st == 0
        pairs = ((A1, M), (B1[:, 0], c0), (C1[0], yrow), (D1[0, 0], yc), (C1[1], urow), (D1[1, 0], uc))
        dev = np.array([np.max(np.abs(g - w)) / (EPS * np.max(np.abs(w))) if np.max(np.abs(w)) > 0 else np.max(np.abs(g)) for g, w in pairs])
        worst = np.maximum(worst, dev)
    with capsys.disabled():
        print(f"\n[connect prototype vs pid_prototype.closed_loop] nx {nx} x {n}: ulp of the largest entry, M {worst[0]:.2f} c0 {worst[1]:.2f} "
              f"yrow {worst[2]:.2f} yc {worst[3]:.2f} urow {worst[4]:.2f} uc {worst[5]:.2f}", end="")
    assert worst.max() <= 4.0, worst


def test_the_ill_posed_pid_case():
    """1 / (s + 1) - 0.5 with p = (2, 0, 0, 0.01): 1 + d (k_p + k_d / tau_f) = 0"""
    plant = (np.array([[-1.0]]), np.array([[1.0]]), np.array([[1.0]]), np.array([[-0.5]]))
    out = proto.unity_feedback(plant, proto.pid((2.0, 0.0, 0.0, 0.01)))
    assert out[4] == proto.ILL_POSED and all(np.isnan(m).all() for m in out[:4])
    out = proto.unity_feedback(plant, proto.pid((2.0, np.nan, 0.0, 0.01)))
    assert out[4] == proto.NOT_FINITE


# ---- the generator of the GPU tests: float64 against longdouble -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", proto.SHAPES, ids=lambda s: "/".join(map(str, s)))
def test_float64_stays_within_1e_14_of_longdouble(shape, capsys):
    """on the very systems tests/test_gpu_connect.py runs (proto.sides: N_SYS systems per shape, one draw of the generator). The condition is
    one on the inputs: a block of a single entry formed by a cancelling sum can miss it for an individual draw (D' of 8/1/2/1/8/1/9/1/1 is
    1 x 1, three terms of order 1: a draw with D' = -0.002 sits at 1.7e-14), so it is asserted where it is relied on."""
    cs, f, l = proto.sides(shape)
    assert (f[4] == 0).all() and (l[4] == 0).all()
    worst = max(float(proto.block_dev(f[k], l[k]).max()) for k in range(4))
    P, Cc, jz, F, G, iz = cs
    cond = 0.0
    for i in range(F.shape[0]):
        D = proto.stack(tuple(m[i] for m in P), None if Cc is None else tuple(m[i] for m in Cc))[3]
        cond = max(cond, float(np.linalg.cond(np.eye(F.shape[1]) - F[i] @ D[jz])))
    with capsys.disabled():
        print(f"\n[connect prototype, float64 vs longdouble] {'/'.join(map(str, shape))} x {F.shape[0]} systems: {worst:.2e} of the block's largest "
              f"entry; cond(E) <= {cond:.2f}", end="")
    assert len(set(jz.tolist())) == len(jz) and len(set(iz.tolist())) == len(iz)
    assert cond <= 3.0 + 1e-9
    assert worst <= 1e-14
