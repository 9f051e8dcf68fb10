"""Parity against output of the Julia reference ITSELF, the day it exists.

tools/gen_golden.jl (run by anyone with Julia 1.12 + Flight.jl) writes tests/golden/julia/*.f64; when those files are present these
tests compare the CPU oracle AND the GPU path with them at the north star's tolerance (1e-6 relative, floors of SURVEY.md §8d).
Until then they skip with that message — parity against the reference stays "unpinned at trajectory level"  — while
`test_consumer_round_trip` keeps the consuming side honest with stand-in files written from the oracle's own config-1 run."""
import os
import numpy as np
import pytest

from golden import from_julia
from support import state_scale

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SKIP = ("no Julia-generated fixtures in tests/golden/julia/ (run `julia --project tools/gen_golden.jl tests/golden/julia` in a Flight.jl "
        "checkout); parity is checked against the C++ oracle only")
TOL = 1e-6


def oracle_config1(oracle, x0=None):
    """config 1 (single Cessna172Sv0, C172.TrimParameters(), dt = 0.01, 10 s) on the oracle; from `x0` when given"""
    g = np.load(os.path.join(GOLDEN, "c172s0_config1.npz"))
    env = oracle.default_env()
    r = oracle.trim(g["trim_params"], np.array([0.1, 0.0, 0.75, 0.47, 0.014, -0.0015, 0.02])[:, None], env)
    assert r["ok"].all()
    start = r["x"] if x0 is None else np.asarray(x0, dtype=np.float64).reshape(27, 1)
    xf, sf, st, traj = oracle.step(start, r["u"], r["ui"], r["s"], env, 0.01, 1000, save_every=100)
    xd, _, _ = oracle.f_ode(xf, r["u"], r["ui"], sf, env)
    return dict(x0=r["x"][:, 0], traj=traj[:, :, 0], xdot_end=xd[:, 0], u=r["u"], ui=r["ui"], s=r["s"])


def compare_config1(ref: dict, got: dict, what: str):
    """ref: from_julia.load(); got: x0 [27], traj [11, 27], xdot_end [27] of the implementation under test"""
    e0 = np.abs(got["x0"] - ref["x0"]) / state_scale(ref["x0"])
    assert e0.max() < TOL, f"{what}: trim state differs from the reference by {e0.max():.3e} (row {e0.argmax()})"
    et = np.abs(got["traj"] - ref["traj"]) / state_scale(ref["traj"].T).T
    assert et.max() < TOL, f"{what}: trajectory differs from the reference by {et.max():.3e} at (sample, row) {np.unravel_index(et.argmax(), et.shape)}"
    if "xdot_end" in ref:
        ed = np.abs(got["xdot_end"] - ref["xdot_end"]) / np.maximum(np.abs(ref["xdot_end"]), 1.0)
        assert ed.max() < 1e-5, f"{what}: xdot at t_end differs by {ed.max():.3e}"


def test_consumer_round_trip(oracle, tmp_path):
    """the loader and the comparison, exercised with stand-in files in Julia's format (column-major raw Float64)"""
    o = oracle_config1(oracle)
    from_julia.write_like_julia(str(tmp_path), x0=o["x0"], traj=o["traj"], xdot_end=o["xdot_end"])
    ref = from_julia.load(str(tmp_path))
    assert set(ref) == {"x0", "traj", "xdot_end"} and ref["traj"].shape == (11, 27)
    compare_config1(ref, o, "oracle vs its own stand-in")
    bad = dict(o); bad["traj"] = o["traj"].copy(); bad["traj"][5, 24] *= 1 + 1e-5
    with pytest.raises(AssertionError, match="trajectory differs"):
        compare_config1(ref, bad, "perturbed")
    with pytest.raises(ValueError, match="expected"):
        np.zeros(5).tofile(os.path.join(str(tmp_path), "traj.f64")); from_julia.load(str(tmp_path))


@pytest.mark.skipif(not {"x0", "traj"} <= set(from_julia.available()), reason=SKIP)
def test_oracle_matches_julia_reference(oracle):
    ref = from_julia.load()
    compare_config1(ref, oracle_config1(oracle), "CPU oracle, own trim")
    compare_config1(ref, oracle_config1(oracle, x0=ref["x0"]), "CPU oracle, from the reference's x0")


@pytest.mark.gpu
@pytest.mark.skipif(not {"x0", "traj"} <= set(from_julia.available()), reason=SKIP)
def test_gpu_matches_julia_reference(fb):
    ref = from_julia.load()
    w = fb.BatchedWorld(64)
    fb.f_init(w, fb.TrimParameters())
    x0 = w.x
    sim = fb.Simulation(w, dt=0.01, t_end=10.0, saveat=1.0)
    fb.init(sim); fb.run(sim)
    ts = fb.TimeSeries(sim)
    xd = np.zeros((27, 64)); fb.f_ode(w, xd)
    compare_config1(ref, dict(x0=x0[:, 0], traj=ts.x[:, :, 0], xdot_end=xd[:, 0]), "GPU (libflightbatch)")
    w.close()


@pytest.mark.gpu
@pytest.mark.skipif("x2_traj" not in from_julia.available(), reason=SKIP)
def test_gpu_x2_matches_julia_reference(fb):
    """Cessna172Xv2, README example 2 (wind N = 1, E = 0.5; EAS_clm with clm_ref = 2; φ_β with φ_ref = 30°), 20 s, every 2 s"""
    ref = from_julia.load()["x2_traj"]
    w = fb.Cessna172Xv2World(64)
    w.set_params(wind_ned=(1.0, 0.5, 0.0))
    sim = fb.Simulation(w, dt=0.01, Δt=0.02, t_end=20.0, saveat=2.0)
    fb.init(sim, fb.TrimParameters())
    w.ctl.lon.mode_req = float(fb.ModeControlLon.EAS_clm); w.ctl.lon.clm_ref = 2.0
    w.ctl.lat.mode_req = float(fb.ModeControlLat.φ_β); w.ctl.lat.φ_ref = float(np.deg2rad(30.0))
    fb.run(sim)
    got = fb.TimeSeries(sim).x[:, :, 0]
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    assert err.max() < TOL, f"GPU Xv2 trajectory differs from the reference by {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    w.close()
