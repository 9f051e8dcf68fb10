"""LQR design on the device, host side (no GPU compute): fb_lqr and fb_lss_get_model are declared, exported, bound and wrapped; the numpy
restatement of the kernel's algorithm (tests/lqr_prototype.py) agrees with scipy's Schur solver on the systems the GPU tests design — the
precondition that makes scipy their yardstick — and flags the three systems without a stabilising solution; closed_loop is A - B K, C - D K."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lqr_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fb_lqr", "fb_lss_get_model")


def test_new_symbols_are_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/flightbatch.h"
        assert re.search(rf"\bT {name}\b", out), f"{name} is not an exported text symbol"
        assert name in fb.EXPORTED and getattr(fb.lib, name).argtypes is not None
        assert f"(:{name}, lib)" in shim, f"the Julia shim has no ccall wrapper for {name}"
    assert len(fb.lib.fb_lqr.argtypes) == 8
    assert (fb.K["FB_LQR_NOT_CONVERGED"], fb.K["FB_LQR_SINGULAR"], fb.K["FB_LQR_NX_MAX"]) == (1, 2, 16)
    assert (proto.NOT_CONVERGED, proto.SINGULAR) == (fb.K["FB_LQR_NOT_CONVERGED"], fb.K["FB_LQR_SINGULAR"])
    for name in ("lqr", "closed_loop", "LqrResult"):
        assert hasattr(fb, name)
    assert hasattr(fb.LinearWorld, "model")


def test_null_handles_are_refused(fb):
    assert fb.lib.fb_lqr(None, *([None] * 7)) != 0 and b"null handle" in fb.lib.fb_last_error()
    assert fb.lib.fb_lss_get_model(None, None, None) != 0 and b"null handle" in fb.lib.fb_last_error()


@pytest.mark.parametrize("nx,nu", proto.SHAPES)
def test_prototype_agrees_with_scipy(nx, nu, capsys):
    A, B, Q, R = proto.systems(nx, nu, 130)
    got = proto.lqr_batch(A, B, Q, R)
    Ks, Xs = proto.scipy_batch(A, B, Q, R)
    dK, dX = proto.rel_dev(got["K"], Ks), proto.rel_dev(got["X"], Xs)
    with capsys.disabled():
        print(f"\n[lqr prototype vs scipy] ({nx:2d}, {nu}) x 130: K {dK:.2e}  X {dX:.2e}  resid <= {got['resid'].max():.2e}  "
              f"iterations {got['iters'].min()} - {got['iters'].max()}", end="")
    assert (got["status"] == 0).all()
    assert dK <= 1e-8 and dX <= 1e-8, (dK, dX)
    assert got["iters"].max() <= 12


def test_prototype_inverse_is_the_inverse():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 22):
        Z = rng.standard_normal((n, n))
        inv, logdet, ok = proto.gj_inverse(Z)
        assert ok and np.abs(inv @ Z - np.eye(n)).max() <= 1e-10
        assert abs(logdet - np.linalg.slogdet(Z)[1]) <= 1e-12 * max(1.0, abs(logdet))


def test_prototype_flags_the_systems_without_a_stabilising_solution():
    for A, B, Q, R, want in proto.failure_systems():
        for a, b, q in ((A, B, Q), proto.embed3(A, B, Q)):
            got = proto.lqr(a, b, q, R)
            assert got["status"] == want, (a, got["status"], want)
            assert np.isnan(got["K"]).all() and np.isnan(got["X"]).all()
            if want == proto.NOT_CONVERGED:
                assert got["iters"] == proto.MAX_ITERS


def test_closed_loop_entry_by_entry(fb):
    A = np.array([[[0.0, 1.0], [-2.0, -3.0]]]); B = np.array([[[0.0], [4.0]]])
    Cm = np.array([[[1.0, 0.0], [0.0, 1.0], [5.0, 6.0]]]); D = np.array([[[0.0], [0.0], [7.0]]])
    Kg = np.array([[[0.5, 0.25]]])
    lss = fb.LinearizedSS(xdot0=np.array([[1.0, 2.0]]), x0=np.array([[3.0, 4.0]]), u0=np.array([[5.0]]), y0=np.array([[6.0, 7.0, 8.0]]),
                          A=A, B=B, C=Cm, D=D, x_labels=("a", "b"), u_labels=("m",), y_labels=("a", "b", "z"))
    cl = fb.closed_loop(lss, Kg)
    assert np.array_equal(cl.A[0], np.array([[0.0, 1.0], [-2.0 - 4.0 * 0.5, -3.0 - 4.0 * 0.25]]))
    assert np.array_equal(cl.C[0], np.array([[1.0, 0.0], [0.0, 1.0], [5.0 - 7.0 * 0.5, 6.0 - 7.0 * 0.25]]))
    assert np.array_equal(cl.xdot0, np.zeros((1, 2)))
    assert np.array_equal(cl.B, B) and np.array_equal(cl.D, D)
    assert np.array_equal(cl.x0, lss.x0) and np.array_equal(cl.u0, lss.u0) and np.array_equal(cl.y0, lss.y0)
    assert cl.x_labels == lss.x_labels and cl.y_labels == lss.y_labels
    assert np.array_equal(fb.closed_loop(lss, Kg[0]).A, cl.A)   # one K for the batch
    assert np.array_equal(lss.A, A)                             # (the model that went in is untouched)
