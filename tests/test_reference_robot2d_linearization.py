"""Robot2D.Vehicle's continuous dynamics — oracle AND HIP path — against numbers the REFERENCE printed and stored.

(1) The reference's design notebook linearises `Robot2D.Vehicle` about rest and prints A (4 x 4), B, C, D to 16 digits
    (lib/FlightApps/design/robot2d/robot2d_design.ipynb cell 2; `linearize`, lib/FlightApps/src/robot2d/robot2d.jl:315-341:
    a finite-difference Jacobian of `f_ode!`'s ẋ and y = (ω, v, θ, η, u_m, τ_m) in x and u). Fixture:
    tests/golden/robot2d_linearization.json (data: the printed matrices). Here: the same Jacobian by Richardson-extrapolated
    central differences of the oracle's `r2_f_ode` and of `fb_f_ode` on a Robot2D handle, held to 1e-9 relative to each
    matrix's largest entry (measured: 1e-12, the noise floor of the difference quotient).
(2) The same notebook's cell 6 designs the velocity loop — LQR with integral action on the η-free model — and its result is
    the reference's robot2d.h5 (K_fbk, K_fwd, K_int; shipped byte-identical, hash-checked). Repeating that design on OUR
    Jacobian (scipy's CARE solver) must give the stored gains, and the printed open- and closed-loop poles."""
import ctypes as C

import numpy as np
import pytest

from reference_fixtures import check_jacobian_and_design
from support import DEFAULT_VP

_D = C.POINTER(C.c_double)


def difference_points(h):
    """records [10, 20]: ±h and ±h/2 about x = 0, u_m = 0 in each of the five directions (ω, v, θ, η | u_m = record row 4)"""
    r = np.zeros((10, 20))
    for j in range(5):
        for k, d in enumerate((h, -h, h / 2, -h / 2)):
            r[j, 4 * j + k] = d
    return r


def jacobian(xd, y, h):
    """[ẋ; y] columns -> A, B, C, D by (4 D(h/2) − D(h)) / 3 (error O(h⁴))"""
    f = np.vstack([xd, y])
    J = np.zeros((f.shape[0], 5))
    for j in range(5):
        c = f[:, 4 * j:4 * j + 4]
        J[:, j] = (4.0 * (c[:, 2] - c[:, 3]) / h - (c[:, 0] - c[:, 1]) / (2 * h)) / 3.0
    return J[:4, :4], J[:4, 4:5], J[4:, :4], J[4:, 4:5]


def test_oracle_robot2d_jacobian_is_the_references(oracle, capsys):
    h = 1e-3
    r = difference_points(h)
    xd = np.zeros((4, 20)); y = np.zeros((6, 20))
    oracle.lib.fo_robot2d_f_ode_y(C.c_int64(20), DEFAULT_VP.ctypes.data_as(_D), r.ctypes.data_as(_D), xd.ctypes.data_as(_D), y.ctypes.data_as(_D))
    with capsys.disabled():
        check_jacobian_and_design(*jacobian(xd, y, h), log=lambda s: print("\n[oracle] " + s, end=""))


@pytest.mark.gpu
def test_device_robot2d_jacobian_is_the_references(fb, capsys):
    """fb_f_ode on a Robot2D handle (k_r2_f_ode<double>) through the C ABI."""
    h = 1e-3
    w = fb.Robot2DWorld(20)
    w.set_state(difference_points(h))
    xd = np.zeros((4, 20))
    fb.f_ode(w, xd)
    y = w.y        # VehicleY: [ω, v, θ, η, u_m, τ_m, ω_dot, v_dot]
    assert np.array_equal(y[6:8], xd[0:2])
    with capsys.disabled():
        check_jacobian_and_design(*jacobian(xd, y[:6], h), log=lambda s: print("\n[HIP] " + s, end=""))
    w.close()
