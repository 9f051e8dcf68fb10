"""Design-model surgery on the device, host side (no GPU compute): fb_lss_transform and fb_lss_steady are declared, exported, bound and
wrapped; fbm::k_transform<8 | 16 | 32> and fbm::k_steady<8 | 16 | 32> are in the library with 0 B of scratch; the refusals that need no
device; the numpy restatement of the kernels (tests/surgery_prototype.py) agrees with np.linalg in float64, reproduces the host surgery of
the tree (reference_lqr.design_model, reference_lqr._k_fwd), and on the generators of the GPU tests its float64 side stays within 1e-14 of
its longdouble side, the condition under which tests/test_gpu_surgery.py's accuracy rule means what it says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surgery_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BLOCKS = ("A'", "B'", "C'", "D'", "xdot0'", "x0'")
S_BLOCKS = ("X", "U", "K_fwd")
ids = lambda s: "/".join(map(str, s))


def test_the_symbols_are_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name, nargs in (("fb_lss_transform", 12), ("fb_lss_steady", 10)):
        assert name in declared
        assert re.search(r"\bT %s\b" % name, out)
        assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == nargs
        assert f"(:{name}, lib)" in shim
    assert re.search(r"^function transform\(w::LinearWorld", shim, flags=re.M) and re.search(r"^function steady_state\(w::LinearWorld", shim, flags=re.M)
    K = fb.K
    assert (K["FB_SURGERY_SINGULAR"], K["FB_SURGERY_NOT_FINITE"], K["FB_SURGERY_N_MAX"]) == (1, 2, 32)
    assert (proto.SINGULAR, proto.NOT_FINITE, proto.N_MAX) == (1, 2, 32)
    sg = fb.surgery
    assert (sg.SINGULAR, sg.NOT_FINITE, sg.N_MAX) == (1, 2, 32)
    for name in ("TransformResult", "SteadyResult", "transform", "subsystem_world", "delete_vars_world", "steady_state", "integrators_world",
                 "integral_augmentation", "lqr_tracker", "c172x_design_model"):
        assert hasattr(fb, name) and getattr(fb, name) is getattr(sg, name)
    # what existed before stays as it was
    assert (K["FB_LQR_NX_MAX"], K["FB_PID_NX_MAX"]) == (16, 28)
    for name in ("integrator_world", "state_feedback", "design_model"):
        assert callable(getattr(fb, name))


def test_the_kernels_are_in_the_library(tmp_path_factory):
    """exactly the instances the dispatchers of the two verbs can launch (csrc/fb_lss.inc: family_launch, group_for), without scratch"""
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    want = {f"fbm::k_{verb}<{P}>" for verb in ("transform", "steady") for P in (8, 16, 32)}
    assert {k for k in ks if k.startswith("fbm::")} == want, sorted(k for k in ks if k.startswith("fbm::"))
    for name in want:
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] <= 160 * 1024, (name, ks[name])
        assert not re.search(r"\bk_step_", name) and "k_lss_" not in name and "k_lqr" not in name
    assert {proto.group(s[0]) for s in proto.T_SHAPES} == {8, 16, 32} == {proto.group(s[0] + s[1]) for s in proto.S_SHAPES}


def test_refusals_that_need_no_device(fb):
    h = C.c_void_p(1)
    one = np.zeros(1, dtype=np.int32)
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = fb.lib.fb_lss_transform(None, pi(one), None, None, 0, None, 0, None, 0, None, None, C.byref(h))
    assert rc != 0 and b"null handle" in fb.lib.fb_last_error() and not h.value
    rc = fb.lib.fb_lss_transform(None, pi(one), None, None, 0, None, 0, None, 0, None, None, None)
    assert rc != 0 and b"fb_lss_transform" in fb.lib.fb_last_error() and b"out is null" in fb.lib.fb_last_error()
    rc = fb.lib.fb_lss_steady(None, pi(one), 1, None, 0, None, None, None, None, None)
    assert rc != 0 and b"null handle" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.transform(object(), [0])
    with pytest.raises(fb.FlightBatchError, match="not a LinearizedSS handle"):
        fb.steady_state(object(), [0])
    with pytest.raises(ValueError, match="valid models"):
        fb.c172x_design_model(object(), model="both")


# ---- the prototype against np.linalg and against the host surgery of the tree --------------------------------------------------------------------
@pytest.mark.parametrize("shape", proto.T_SHAPES, ids=ids)
def test_the_transform_prototype_against_numpy(shape):
    (M, rows, zero, ix, iu, iy), f64, _ = proto.t_sides(shape)
    xdot0, x0, u0, y0, A, B, Cm, D = M
    assert (f64[6] == 0).all()
    for i in (0, 1, proto.N_SYS - 1):
        T = Cm[i][rows]
        Ti = np.linalg.inv(T)
        xd = np.where(zero.astype(bool), 0.0, T @ xdot0[i])
        want = (T @ A[i] @ Ti, T @ B[i], Cm[i] @ Ti, D[i], xd, y0[i][rows])
        for name, g, w in zip(T_BLOCKS, f64[:6], want):
            assert np.abs(g[i] - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0), (name, i)
    assert (f64[4][:, zero.astype(bool)] == 0.0).all() and np.array_equal(f64[3], D) and np.array_equal(f64[5], y0[:, rows])
    assert ((f64[7] > 0) & (f64[7] <= 1)).all()


@pytest.mark.parametrize("shape", proto.S_SHAPES, ids=ids)
def test_the_steady_prototype_against_numpy(shape):
    (M, iz, K, _), f64, _ = proto.s_sides(shape)
    A, B, Cm, D = M
    nx = shape[0]
    assert (f64[3] == 0).all()
    for i in (0, 1, proto.N_SYS - 1):
        Minv = np.linalg.inv(np.block([[A[i], B[i]], [Cm[i][iz], D[i][iz]]]))
        want = (Minv[:nx, nx:], Minv[nx:, nx:], Minv[nx:, nx:] + K[i] @ Minv[:nx, nx:])
        for name, g, w in zip(S_BLOCKS, f64[:3], want):
            assert np.abs(g[i] - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0), (name, i)
    none = proto.steady(tuple(b[0] for b in M), iz)
    assert none[2] is None and np.array_equal(none[0], f64[0][0]) and np.array_equal(none[1], f64[1][0])


def test_the_prototype_reproduces_the_host_surgery_of_the_tree():
    """reference_lqr.design_model (T A inv(T), T B with T = the identity but for the rows of EAS, α, β, n_eng) and reference_lqr._k_fwd"""
    import reference_lqr as rl
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((20, 20)) / np.sqrt(20), rng.standard_normal((20, 4))
    Cy = 0.3 * rng.standard_normal((3, 20))
    for k, lab in enumerate(("v_x", "v_y", "v_z")):
        Cy[k, rl.X_LABELS.index(lab)] += 1.0
    Ap, Bp = rl.design_model(A, B, Cy)
    # the same T as output rows of a model: the 20 states, then EAS, α, β, n_eng
    n_eng = np.zeros((1, 20)); n_eng[0, rl.X_LABELS.index("ω_eng")] = 1.0 / rl.OMEGA_RATED
    Cm = np.vstack([np.eye(20), Cy, n_eng])
    rows = [20 + ("EAS", "α", "β", "n_eng").index(s) if s in ("EAS", "α", "β", "n_eng") else rl.X_LABELS.index(s) for s in rl.XP_LABELS]
    m = (np.zeros(20), np.zeros(20), np.zeros(4), np.zeros(24), A, B, Cm, np.zeros((24, 4)))
    got = proto.transform(m, rows)
    assert got[6] == 0
    assert np.abs(got[0] - Ap).max() <= 1e-13 * np.abs(Ap).max() and np.abs(got[1] - Bp).max() <= 1e-13 * np.abs(Bp).max()
    xl, ul, zl = rl.DESIGNS["tv2te"][:3]
    Ar, Br = rl._sub(Ap, Bp, xl, ul)
    Cz, Dz = rl._z_rows(xl, ul, zl)
    K = rng.standard_normal((2, 8))
    X, U, Kf, st, rpiv = proto.steady((Ar, Br, Cz, Dz), [0, 1], K)
    want = rl._k_fwd(Ar, Br, Cz, Dz, K)
    assert st == 0 and 0 < rpiv <= 1 and np.abs(Kf - want).max() <= 1e-11 * np.abs(want).max()


def test_flagged_systems_of_the_prototype():
    (M, rows, zero, *_), _, _ = proto.t_sides((8, 2, 9, 8, 2, 9))
    one = [b[0].copy() for b in M]
    twice = rows.copy(); twice[3] = twice[5]
    out = proto.transform(one, twice)
    assert out[6] == proto.SINGULAR and out[7] == 0.0 and all(np.isnan(b).all() for b in out[:5]) and np.array_equal(out[5], one[3][twice])
    one[4][2, 2] = np.nan
    out = proto.transform(one, rows)
    assert out[6] == proto.NOT_FINITE and np.isnan(out[7])
    eye = (np.zeros(3), np.zeros(3), np.zeros(1), np.zeros(3), np.ones((3, 3)), np.ones((3, 1)), np.eye(3), np.zeros((3, 1)))
    out = proto.transform(eye, [0, 1, 2])
    assert out[6] == 0 and out[7] == 1.0 and np.array_equal(out[0], eye[4])
    (S, iz, K, _), _, _ = proto.s_sides((6, 2))
    sys0 = [b[0].copy() for b in S]
    sys0[0][:, 3] = 0.0; sys0[2][:, 3] = 0.0          # an all-zero column of L
    out = proto.steady(sys0, iz, K[0])
    assert out[3] == proto.SINGULAR and out[4] == 0.0 and all(np.isnan(b).all() for b in out[:3])


# ---- the generators of the GPU tests: float64 against longdouble -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", proto.T_SHAPES, ids=ids)
def test_transform_float64_stays_within_1e_14_of_longdouble(shape, capsys):
    (M, rows, *_), f, l = proto.t_sides(shape)
    assert (f[6] == 0).all() and (l[6] == 0).all()
    dev = [float(proto.block_dev(f[k], l[k]).max()) for k in range(6)]
    cond = max(float(np.linalg.cond(M[6][i][rows])) for i in range(proto.N_SYS))
    with capsys.disabled():
        print(f"\n[transform prototype, float64 vs longdouble] {ids(shape)} x {proto.N_SYS} systems: " +
              "  ".join(f"{b} {d:.2e}" for b, d in zip(T_BLOCKS, dev)) + f"; cond(T) <= {cond:.2f}", end="")
    assert len(set(rows.tolist())) == len(rows)
    assert max(dev) <= 1e-14


@pytest.mark.parametrize("wide", [False, True], ids=["K per system", "K batch-wide"])
@pytest.mark.parametrize("shape", proto.S_SHAPES, ids=ids)
def test_steady_float64_stays_within_1e_14_of_longdouble(shape, wide, capsys):
    (M, iz, *_), f, l = proto.s_sides(shape, wide)
    assert (f[3] == 0).all() and (l[3] == 0).all()
    dev = [float(proto.block_dev(f[k], l[k]).max()) for k in range(3)]
    A, B, Cm, D = M
    cond = max(float(np.linalg.cond(np.block([[A[i], B[i]], [Cm[i][iz], D[i][iz]]]))) for i in range(proto.N_SYS))
    with capsys.disabled():
        print(f"\n[steady prototype, float64 vs longdouble, {'K batch-wide' if wide else 'K per system'}] {ids(shape)} x {proto.N_SYS} systems: " +
              "  ".join(f"{b} {d:.2e}" for b, d in zip(S_BLOCKS, dev)) + f"; cond(L) <= {cond:.2f}", end="")
    assert max(dev) <= 1e-14
