"""Model(lss) on the device, host side (no GPU compute): the new entry points are declared, exported and bound; fb_lss_create refuses what
it does not support before anything touches a device (so every check here holds with and without a GPU); fb_create points to fb_lss_create;
the Python packing of a LinearizedSS is the (r + rows c) N + i layout fb_linearize writes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fb_lss_create", "fb_lss_set_model", "fb_lss_from_linearization", "fb_lss_exchange")


def test_new_symbols_are_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/flightbatch.h"
        assert re.search(rf"\bT {name}\b", out), f"{name} is not an exported text symbol"
        assert name in fb.EXPORTED and getattr(fb.lib, name).argtypes is not None
    assert fb.K["FB_MODEL_LSS"] == 3
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name in NEW:
        assert f"(:{name}, lib)" in shim, f"the Julia shim has no ccall wrapper for {name}"
    for name in ("LinearWorld", "linear_world"):
        assert hasattr(fb, name)


def test_fb_lss_create_refuses_before_any_device_call(fb):
    h = C.c_void_p()
    for args, msg in (((0, 1, 1, 8, 0), b"nx = 0"), ((33, 1, 1, 8, 0), b"nx = 33"), ((4, 9, 1, 8, 0), b"nu = 9"), ((4, 0, 1, 8, 0), b"nu = 0"),
                      ((4, 1, 65, 8, 0), b"ny = 65"), ((4, 1, 0, 8, 0), b"ny = 0"), ((4, 1, 6, 0, 0), b"n must be positive"),
                      ((4, 1, 6, 8, -1), b"no CPU backend")):
        h.value = 1   # (a refused create hands back NULL, not what was there)
        assert fb.lib.fb_lss_create(*args, C.byref(h)) != 0 and msg in fb.lib.fb_last_error(), (args, fb.lib.fb_last_error())
        assert not h.value
    # the arguments are judged first, the device after them (fb_create's order)
    assert fb.lib.fb_lss_create(33, 1, 1, 8, -1, C.byref(h)) != 0 and b"nx = 33" in fb.lib.fb_last_error()
    assert fb.lib.fb_lss_create(4, 1, 6, 8, 0, None) != 0


def test_fb_create_points_to_fb_lss_create(fb):
    h = C.c_void_p()
    for dev in (0, -1):
        assert fb.lib.fb_create(fb.K["FB_MODEL_LSS"], 0, fb.K["FB_F64"], 8, dev, C.byref(h)) != 0
        assert b"fb_lss_create" in fb.lib.fb_last_error() and not h.value
    assert fb.lib.fb_create(99, 0, fb.K["FB_F64"], 8, 0, C.byref(h)) != 0 and b"unknown model id" in fb.lib.fb_last_error()
    # and the entry points that take a handle say so when they get none
    assert fb.lib.fb_lss_set_model(None, *([None] * 8)) != 0 and b"null handle" in fb.lib.fb_last_error()
    assert fb.lib.fb_lss_from_linearization(None, None, 0, None, 0, None, 0, C.byref(h)) != 0 and b"null handle" in fb.lib.fb_last_error()
    xch = C.c_int32(7)
    assert fb.lib.fb_lss_exchange(None, C.byref(xch)) != 0 and b"fb_lss_exchange" in fb.lib.fb_last_error() and xch.value == 7


def test_packing_round_trips_the_abi_layout(fb):
    from flightbatch import lss as L
    rng = np.random.default_rng(5)
    n, nx, nu, ny = 3, 5, 2, 7
    mk = lambda *s: rng.standard_normal(s)
    m = fb.LinearizedSS(xdot0=mk(n, nx), x0=mk(n, nx), u0=mk(n, nu), y0=mk(n, ny), A=mk(n, nx, nx), B=mk(n, nx, nu), C=mk(n, ny, nx),
                        D=mk(n, ny, nu), x_labels=tuple("abcde"), u_labels=("p", "q"), y_labels=tuple("tuvwxyz"))
    b = L.pack_model(m)
    for key, rows, cols in (("A", nx, nx), ("B", nx, nu), ("C", ny, nx), ("D", ny, nu)):
        flat, M = b[key], getattr(m, key)
        assert flat.shape == (rows * cols * n,) and flat.flags.c_contiguous and flat.dtype == np.float64
        for i in range(n):
            for r in range(rows):
                for c in range(cols):
                    assert flat[(r + rows * c) * n + i] == M[i, r, c]
        assert np.array_equal(L.unpack_matrix(flat, rows, cols), M)
        # the layout flightbatch.linearization reads fb_linearize's blocks with
        assert np.array_equal(flat.reshape(cols, rows, n).transpose(2, 1, 0), M)
    for key, rows in (("xdot0", nx), ("x0", nx), ("u0", nu), ("y0", ny)):
        v = b[key]
        assert v.shape == (rows, n) and v.flags.c_contiguous
        assert np.array_equal(v.reshape(-1)[np.arange(rows)[:, None] * n + np.arange(n)[None, :]], getattr(m, key).T)


def test_lss_and_lqr_kernels_are_in_the_library(tmp_path_factory):
    """the instances lss_with_group and the LQR dispatcher launch, with the scratch and LDS docs/design/linearize.md tabulates"""
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    where = "the table of instances is the docstring of tests/test_gpu_lss_instances.py: an instance added or removed gets its row there"
    groups = (4, 8, 16, 32)
    lds = {f"fbl::k_lss_rk4<{g}, {x}>": 2048 * (1 - x) for g in groups for x in (0, 1)}
    lds.update({f"fbl::k_lss_f_ode<{g}>": 2048 for g in groups})
    lds["fbl::k_lss_gather"] = 0
    assert {k for k in ks if k.startswith("fbl::k_lss_")} == set(lds), where
    lqr = {f"fbq::k_lqr<{g}>" for g in (8, 16, 32)}
    assert {k for k in ks if k.startswith("fbq::k_lqr")} == lqr, where
    for name in sorted(set(lds) | lqr):
        assert ks[name]["scratch"] == 0, (name, ks[name], where)
    for name, want in lds.items():
        assert ks[name]["lds"] == want, (name, ks[name], where)
