"""A stepping-kernel lane that takes atan2_tab OUTSIDE its domain, against the oracle: aircraft set (fb_set_state) so close to the north pole
that n_x and n_y are both non-zero and below 1e-30 — fp32 denormals, where the single-precision estimate of atan2_tab's quotient is
infinite or NaN. The longitude the stepping kernels then compute for the geoid lookup is wrong but bounded (tests/math_cases.py, SPECIALS)
and its table read stays inside the table (the index is clamped); at the pole the geoid does not depend on the longitude, so the
trajectory must agree with the oracle as everywhere else. Lanes a tenth of a degree away share the waves and are the control.
The criterion is smoke()'s: 100 RK4 steps, max |x - x_oracle| / max(|x_oracle|, 1) < 1e-6."""
import numpy as np
import pytest

from support import flying_batch, stepper

pytestmark = pytest.mark.gpu
N = 96   # a full wave and a ragged one


def pole_batch(fb, oracle):
    rng = np.random.default_rng(90)
    lat, lon = np.deg2rad(rng.uniform(89.85, 89.95, N)), rng.uniform(-np.pi, np.pi, N)
    x, s, u, ui = flying_batch(fb, oracle, N, 90, lat, lon, rng.uniform(800.0, 1500.0, N), np.zeros(N), {})
    pole = np.arange(N) % 3 == 0
    t = rng.uniform(-np.pi, np.pi, N)
    tiny = rng.choice(np.array([1e-41, -1e-41, 3e-43, 2e-38, 7e-32]), N)
    q = np.stack([tiny, np.cos(t), np.sin(t), np.where(np.arange(N) % 2 == 0, 0.0, 0.5 * tiny)])
    x[16:20, pole] = q[:, pole]
    # what the kernel forms from q_ew (n_e, csrc/c172_device_impl.inc): both horizontal components non-zero and below atan2_tab's domain
    w_, x_, y_, z_ = x[16:20]
    n_x, n_y = -(2 * x_ * z_ + 2 * w_ * y_), -(2 * y_ * z_ - 2 * w_ * x_)
    mx = np.maximum(np.abs(n_x), np.abs(n_y))
    assert (mx[pole] > 0).all() and (mx[pole] < 1e-30).all() and (np.minimum(np.abs(n_x), np.abs(n_y))[pole] > 0).all()
    assert (mx[~pole] > 1e-4).all()
    return x, s, u, ui, pole


@pytest.mark.parametrize("duo", [True, False])
def test_lanes_at_the_pole_against_the_oracle(fb, oracle, duo):
    x0, s0, u0, ui0, pole = pole_batch(fb, oracle)
    with stepper(duo):
        w = fb.BatchedWorld(N)
        w.set_state(x0, s0); w.u = u0; w.ui = ui0
        sim = fb.Simulation(w, dt=0.01, save_on=False, steps_per_launch=20)
        fb.step(sim, 1.0); w.sync()
        xg, st = w.x, w.status
        w.close()
    xo, so, sto = oracle.step(x0, u0, ui0, s0, oracle.default_env(), 0.01, 100)
    err = np.max(np.abs(xg - xo) / np.maximum(np.abs(xo), 1.0), axis=0)
    print("\n[%s] max scaled |x - x_oracle| after 100 steps: lanes at the pole %.3e, control lanes %.3e"
          % ("k_step_duo" if duo else "k_step_air", err[pole].max(), err[~pole].max()), end="")
    assert np.isfinite(xg).all() and (st == 0).all() and (sto == 0).all()
    assert err.max() < 1e-6, (err[pole].max(), err[~pole].max())
