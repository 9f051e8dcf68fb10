"""fb_linearize's host side, no GPU: the ABI declares and exports the verbs, the library carries their kernels without scratch, the
Python labels are the reference's (FA/c172/c172s/c172s.jl:269-299, FA/c172/c172x/c172x.jl:332-370, FA/robot2d/robot2d.jl:233-256), and
subsystem / delete_vars behave as FP/linearization.jl:113-148."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flightbatch.h")
VERBS = ("fb_linearize", "fb_linearize_state", "fb_linearize_dims")


def _pkg():
    import __graft_entry__ as g
    g.build()
    sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd"))
    import flightbatch
    return flightbatch


def test_header_declares_and_library_exports_the_verbs():
    text = open(HEADER).read()
    for v in VERBS:
        assert re.search(r"int32_t\s+%s\(" % v, text), v
    assert re.search(r"FB_LIN_FORWARD\s*=\s*0", text) and re.search(r"FB_LIN_ONESIDED2\s*=\s*1", text)
    fb = _pkg()
    for v in VERBS:
        assert v in fb.EXPORTED and hasattr(fb.lib, v)
    assert fb.K["FB_LIN_FORWARD"] == 0 and fb.K["FB_LIN_ONESIDED2"] == 1


def test_kernels_are_in_the_library_without_scratch(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    want = ["fbd::k_lin_base<false>", "fbd::k_lin_base<true>", "fbr::k_r2_lin_base"]
    want += [f"fbd::k_lin_diff<{x}, 0, 0>" for x in ("false", "true")]
    want += [f"fbd::k_lin_diff<{x}, 1, {p}>" for x in ("false", "true") for p in (0, 1)]
    want += ["fbr::k_r2_lin_diff<0>", "fbr::k_r2_lin_diff<1>"]
    for name in want:
        assert name in ks, (name, sorted(k for k in ks if "lin" in k))
        assert ks[name]["scratch"] == 0, (name, ks[name])


def test_labels_are_the_references():
    from flightbatch.linearization import LABELS
    _pkg()
    lens = {"FB_MODEL_C172S0": (16, 4, 33), "FB_MODEL_C172X2": (20, 4, 38), "FB_MODEL_ROBOT2D": (4, 1, 6)}
    for m, (nx, nu, ny) in lens.items():
        x, u, y = LABELS[m]
        assert (len(x), len(u), len(y)) == (nx, nu, ny), m
        assert len(set(x)) == nx and len(set(u)) == nu and len(set(y)) == ny
    x, u, y = LABELS["FB_MODEL_C172S0"]
    assert x == ("p", "q", "r", "ψ", "θ", "φ", "v_x", "v_y", "v_z", "ϕ", "λ", "h", "α_filt", "β_filt", "ω_eng", "fuel")
    assert u == ("throttle", "aileron", "elevator", "rudder")
    assert y[:16] == x and y[16:] == ("f_x", "f_y", "f_z", "α", "β", "EAS", "TAS", "v_N", "v_E", "v_D", "χ", "γ", "c",
                                      "throttle_out", "aileron_out", "elevator_out", "rudder_out")
    x, u, y = LABELS["FB_MODEL_C172X2"]
    import reference_lqr as rl
    assert x == tuple(rl.X_LABELS) and u == tuple(rl.U_LABELS)
    assert y[14:21] == ("ω_eng", "n_eng", "fuel", "thr_p", "ail_p", "ele_p", "rud_p") and y[-5:] == ("climb_rate",) + u
    assert LABELS["FB_MODEL_ROBOT2D"] == (("ω", "v", "θ", "η"), ("m",), ("ω", "v", "θ", "η", "u_m", "τ_m"))


def _synthetic(n=3):
    from flightbatch.linearization import LinearizedSS
    rng = np.random.default_rng(0)
    xl, ul, yl = ("a", "b", "c"), ("u1", "u2"), ("a", "y1", "u1", "y2")
    return LinearizedSS(xdot0=rng.normal(size=(n, 3)), x0=rng.normal(size=(n, 3)), u0=rng.normal(size=(n, 2)), y0=rng.normal(size=(n, 4)),
                        A=rng.normal(size=(n, 3, 3)), B=rng.normal(size=(n, 3, 2)), C=rng.normal(size=(n, 4, 3)), D=rng.normal(size=(n, 4, 2)),
                        x_labels=xl, u_labels=ul, y_labels=yl, status=np.zeros(n, np.int32))


def test_subsystem_and_delete_vars():
    _pkg()
    from flightbatch.linearization import subsystem, delete_vars
    s = _synthetic()
    sub = subsystem(s, x=["c", "a"], u=["u2"], y=["y2", "a"])
    assert sub.x_labels == ("c", "a") and sub.u_labels == ("u2",) and sub.y_labels == ("y2", "a")
    assert np.array_equal(sub.A, s.A[:, [2, 0]][:, :, [2, 0]]) and np.array_equal(sub.B, s.B[:, [2, 0]][:, :, [1]])
    assert np.array_equal(sub.C, s.C[:, [3, 0]][:, :, [2, 0]]) and np.array_equal(sub.D, s.D[:, [3, 0]][:, :, [1]])
    assert np.array_equal(sub.xdot0, s.xdot0[:, [2, 0]]) and np.array_equal(sub.y0, s.y0[:, [3, 0]]) and np.array_equal(sub.u0, s.u0[:, [1]])
    full = subsystem(s)   # keyword defaults: everything, in order
    for k in ("A", "B", "C", "D", "x0", "y0"):
        assert np.array_equal(getattr(full, k), getattr(s, k))
    # a name leaves every axis it is on ("a" is a state and an output, "u1" an input and an output)
    d = delete_vars(s, ["a", "u1"])
    assert d.x_labels == ("b", "c") and d.u_labels == ("u2",) and d.y_labels == ("y1", "y2")
    assert np.array_equal(d.A, s.A[:, [1, 2]][:, :, [1, 2]]) and np.array_equal(d.D, s.D[:, [1, 3]][:, :, [1]])
    assert delete_vars(s, "b").x_labels == ("a", "c")
    with pytest.raises(KeyError):
        subsystem(s, x=["nope"])
