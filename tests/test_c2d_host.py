"""Sampled models on the device, host side (no GPU compute): fb_lss_c2d and fb_lss_sample_time are declared, exported, bound and wrapped;
fbz::k_lss_c2d<8 | 16 | 32>, fbz::k_lss_map<4 | 8 | 16 | 32, 0 | 1> and fbz::k_timeresp_map<8 | 16 | 32> are in the library with 0 B of scratch;
the refusals that need no device; the numpy restatement of the kernels (tests/c2d_prototype.py) is held to the exact side
(scipy.linalg.expm of [[A, B, xdot0], [0]] Ts) over the GPU tests' cases, which are checked to be fair; and on every pair the sampled
StepInfo test uses, the indices from the prototype's samples equal those from the exact samples, every deciding sample at least 1e-9 of
the step size from its threshold — the condition under which tests/test_gpu_c2d.py may ask for equal indices.

The prototype's own bound: with |Z|_inf <= 1/2 the series is cut below 2^-17 / 18! of its sum, each product of row length nx adds at most
nx rounding errors of 2^-53 relative to the largest entry, and each squaring at most doubles what is there: 2^s max(nx, 4) 2^-52 of the
block's largest exact entry."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import c2d_prototype as proto
import timeresp_prototype as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_MIN = 1e-9


def test_the_symbols_are_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name, nargs in (("fb_lss_c2d", 5), ("fb_lss_sample_time", 2)):
        assert name in declared
        assert re.search(r"\bT %s\b" % name, out)
        assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == nargs
    assert "(:fb_lss_c2d, lib)" in shim and re.search(r"^function c2d\(w::LinearWorld", shim, flags=re.M)
    assert (fb.K["FB_C2D_NOT_FINITE"], fb.K["FB_C2D_RANGE"], fb.K["FB_C2D_SQUARINGS_MAX"]) == (1, 2, 30)
    assert (proto.NOT_FINITE, proto.RANGE, proto.SQUARINGS_MAX) == (1, 2, 30)
    assert callable(fb.c2d) and callable(fb.lsim) and fb.lsim is fb.timeresp.lsim and hasattr(fb, "C2dResult")
    import inspect
    for f in (fb.timeresp.step, fb.timeresp.stepinfo):
        assert inspect.signature(f).parameters["method"].default == "rk4"


def test_the_kernels_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    want = {f"fbz::k_lss_c2d<{P}>": (P * P + 10 * P) * (64 // P) * 8 for P in (8, 16, 32)}          # a full factor and the thin block per group
    want.update({f"fbz::k_lss_map<{G}, {x}>": 2048 * (1 - x) for G in (4, 8, 16, 32) for x in (0, 1)})
    want.update({f"fbz::k_timeresp_map<{P}>": 512 for P in (8, 16, 32)})
    assert {k for k in ks if k.startswith("fbz::")} == set(want), sorted(k for k in ks if k.startswith("fbz::"))
    for name, lds in want.items():
        print(name, ks[name])
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == lds, (name, ks[name])


def test_refusals_that_need_no_device(fb):
    h, ts = C.c_void_p(), C.c_double(-1.0)
    assert fb.lib.fb_lss_c2d(None, 0.01, None, None, C.byref(h)) != 0 and b"null handle" in fb.lib.fb_last_error() and not h.value
    assert fb.lib.fb_lss_c2d(None, 0.01, None, None, None) != 0 and b"out is null" in fb.lib.fb_last_error()
    assert fb.lib.fb_lss_sample_time(None, C.byref(ts)) != 0 and b"null handle" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError, match="LinearWorld"):
        fb.c2d(object(), 0.01)


# ---- the prototype against the exact side over the GPU test's cases, and the cases themselves ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(nx, nu, Ts):
    M = proto.plants(nx, nu)
    return M, proto.c2d_batch(M[4], M[5], M[0], Ts), proto.exact_batch(M[4], M[5], M[0], Ts)


@pytest.mark.parametrize("Ts", proto.TS_ALL)
@pytest.mark.parametrize("nx", proto.NX_ALL)
def test_prototype_against_the_exact_side_on_fair_cases(nx, Ts, capsys):
    worst, s_max, nrm, phi_min = 0.0, 0, 0.0, np.inf
    for nu in proto.NU_ALL:
        M, got, ex = _case(nx, nu, Ts)
        assert (got[4] == 0).all()
        worst, s_max = max(worst, proto.worst_dev(got[:3], ex)), max(s_max, int(got[3].max()))
        for i in range(proto.N_SYS):
            a, p = proto.fair(M[4][i], ex[0][i], Ts)
            nrm, phi_min = max(nrm, a), min(phi_min, p)
            s = int(got[3][i])
            assert a / 2.0 ** s <= 0.5 * (1 + 1e-12) and (s == 0 or a / 2.0 ** (s - 1) > 0.5 * (1 - 1e-12))      # the smallest s with a / 2^s <= 1/2
    with capsys.disabled():
        print(f"\n[c2d prototype vs expm] nx {nx:2d}, Ts {Ts:g}, nu {proto.NU_ALL} x {proto.N_SYS} systems: worst block deviation {worst:.2e}; "
              f"s <= {s_max}; |A|_inf Ts <= {nrm:.3f}; max|Phi| >= {phi_min:.3f}", end="")
    assert nrm <= proto.NORM_MAX and s_max <= 9 and phi_min >= proto.PHI_MIN
    assert worst <= 2.0 ** s_max * max(nx, 4) * 2.0 ** -52


@pytest.mark.parametrize("nx", [7, 17])
def test_the_scaled_plants_square_differently_within_a_wave(nx, capsys):
    M = proto.scaled(nx)
    s = proto.c2d_batch(M[4], M[5], M[0], 0.25)[3]
    with capsys.disabled():
        print(f"\n[c2d prototype, one plant times 1, 8, 64] nx {nx}: s {s.tolist()}", end="")
    assert len(set(s[:3].tolist())) == 3 and (s[3:6] == s[:3]).all() and (s[1:3] - s[0] == (3, 6)).all() and s.max() <= 9


def test_singular_unstable_and_failing_systems(capsys):
    one = lambda v: np.array(v, dtype=np.float64)
    for name, A, B in (("integrator chain", one([[0, 1], [0, -2]]), one([[0], [1]])), ("1 / (s - 20)", one([[20]]), one([[1]]))):
        xd = np.ones(A.shape[0])
        Phi, Gam, dl, s, st = proto.c2d(A, B, xd, 0.01)
        ex = proto.exact(A, B, xd, 0.01)
        dev = max(np.abs(g - e).max() / np.abs(e).max() for g, e in zip((Phi, Gam, dl), ex))
        with capsys.disabled():
            print(f"\n[c2d prototype, {name}] Ts 0.01: s {s}, status {st}, worst block deviation {dev:.2e}", end="")
        assert st == 0 and dev <= 4 * 2.0 ** -52
    A = np.eye(3)
    A[1, 2] = np.nan
    assert proto.c2d(A, np.ones((3, 1)), np.zeros(3), 0.01)[3:] == (0, proto.NOT_FINITE)
    Phi, Gam, dl, s, st = proto.c2d(1e12 * np.eye(2), np.ones((2, 1)), np.zeros(2), 1.0)
    assert (s, st) == (0, proto.RANGE) and np.isnan(Phi).all() and np.isnan(Gam).all() and np.isnan(dl).all()
    assert proto.c2d(one([[2000.0]]), one([[1.0]]), one([0.0]), 1.0)[3:] == (0, proto.NOT_FINITE)          # e^2000 overflows


# ---- the sampled stepper and lsim ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", proto.STEP_NX)
def test_map_steps_against_the_exact_trajectory(nx, capsys):
    xd0, x0, u0, y0, A, B, Cm, D = proto.plants(nx, 2)
    Phi, Gam, dl = proto.c2d_batch(A, B, xd0, proto.STEP_TS)[:3]
    Phe, Gae, dle = proto.exact_batch(A, B, xd0, proto.STEP_TS)
    u = u0.copy()
    u[:, 1] += 1.0
    x, xe, worst = x0.copy(), x0.copy(), 0.0
    for k in range(proto.STEP_N // proto.STEP_EVERY):
        x = proto.map_steps(Phi, Gam, dl, x0, u0, x, u, proto.STEP_EVERY)
        xe = proto.map_steps(Phe, Gae, dle, x0, u0, xe, u, proto.STEP_EVERY)
        y, ye = proto.outputs(Cm, D, x0, u0, y0, x, u), proto.outputs(Cm, D, x0, u0, y0, xe, u)
        worst = max(worst, float((np.abs(y - ye) / np.maximum(np.abs(ye), 1.0)).max()))
    with capsys.disabled():
        print(f"\n[map stepper prototype vs exact map] nx {nx}, {proto.STEP_N} steps of {proto.STEP_TS}: outputs {worst:.2e} of max(|y|, 1)", end="")
    assert worst <= 1e-12


def test_lsim_prototype_carries_the_new_input_at_a_change():
    one = lambda v: np.array(v, dtype=np.float64)
    Phi, Gam, dl = one([[[0.5]]]), one([[[1.0]]]), one([[0.0]])
    Cm, D, z = one([[[1.0]]]), one([[[10.0]]]), np.zeros((1, 1))
    U = one([0, 0, 1, 1]).reshape(4, 1, 1)
    y, x = proto.lsim(Phi, Gam, dl, Cm, D, z, z, z, z.copy(), U)
    assert y[:, 0, 0].tolist() == [0.0, 0.0, 10.0, 11.0] and x[:, 0, 0].tolist() == [0.0, 0.0, 0.0, 1.0]


# ---- the sampled StepInfo: the same indices from the prototype's samples and from the exact ones, with the margins --------------------------------------
@pytest.mark.parametrize("nx", tr.NX_ALL)
def test_sampled_stepinfo_indices_and_margins(nx, capsys):
    _, P, Pe = proto.stepinfo_case(nx)
    N = int(round(proto.SI_TSIM / proto.SI_TS))
    Y, Ye = proto.samples_map(*P, N), proto.samples_map(*Pe, N)
    dev = tr.sample_dev(Y, Ye)
    worst = {}
    for name, (y0_in, yf_in, opts) in tr.gpu_variants(tr.pairs(*tr.plants(nx), tr.CHANNELS), Ye).items():
        info, status = tr.stepinfo_batch(Y, proto.SI_TS, y0_in, yf_in, opts)
        info_e, status_e = tr.stepinfo_batch(Ye, proto.SI_TS, y0_in, yf_in, opts)
        assert (status == 0).all() and (status_e == 0).all(), name
        assert np.array_equal(info[[4, 7, 8]], info_e[[4, 7, 8]], equal_nan=True), name
        ms = [tr.margins(Ye[:, p], None if y0_in is None else y0_in[p], None if yf_in is None else yf_in[p], opts) for p in range(Y.shape[1])]
        worst[name] = min(min(m.values()) for m in ms)
    with capsys.disabled():
        print(f"\n[sampled stepinfo prototype vs exact] nx {nx:2d} x {Y.shape[1]} pairs, N {N}: samples {dev.max():.2e} of max|y|; smallest margin of "
              "the exact side " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()), end="")
    # the blocks of the map are within max(nx, 4) 2^-52 of the exact ones (s = 0 at this Ts, above) and a step's own sums round as much again;
    # the plants do not expand (A + A' < 0), so over N steps the errors add at most linearly
    assert dev.max() <= 2 * N * max(nx, 4) * 2.0 ** -52
    assert min(worst.values()) >= MARGIN_MIN, worst
