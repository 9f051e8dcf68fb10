"""Step responses on the device, host side (no GPU compute): fb_lss_stepinfo is declared, exported, bound and wrapped; fbt::k_timeresp<8 | 16 | 32>
are in the library with 0 B of scratch; the refusals that need no device; the numpy restatement of the kernel (tests/timeresp_prototype.py)
reproduces the two StepInfo tables the reference's robot2d design notebook stores, line for line in show's format, and agrees with exact
discretisation on the systems the GPU tests use; and on every pair the GPU tests use, every deciding sample sits at least 1e-9 of the step
size from its threshold — the condition under which tests/test_gpu_timeresp.py may ask for equal indices."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import timeresp_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_MIN = 1e-9


def test_the_symbol_is_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name, nargs in (("fb_lss_stepinfo", 13), ("fb_lss_stepinfo_samples", 2)):
        assert name in declared
        assert re.search(r"\bT %s\b" % name, out)
        assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == nargs
    assert "(:fb_lss_stepinfo, lib)" in shim and re.search(r"^function stepinfo\(w::LinearWorld", shim, flags=re.M)
    assert (fb.K["FB_STEPINFO_DIVERGED"], fb.K["FB_STEPINFO_FLAT"], fb.K["FB_STEPINFO_NX_MAX"]) == (1, 2, 31)
    assert (proto.DIVERGED, proto.FLAT, proto.NX_MAX) == (1, 2, 31)
    T = fb.timeresp
    assert (T.DIVERGED, T.FLAT, T.NX_MAX) == (1, 2, 31) and T.FIELDS == proto.FIELDS
    for name in ("timeresp", "stepinfo", "StepInfo", "StepResult"):
        assert hasattr(fb, name)
    assert callable(T.step) and callable(T.stepinfo) and fb.stepinfo is T.stepinfo


def test_the_sample_count_is_one_formula(fb):
    for nsteps, stride in ((1, 1), (2000, 1), (2000, 7), (2000, 2000), (2000, 1999), (2000, 2001), (200000, 3), (5, 2147483647)):
        want = -(-nsteps // stride) + 1
        assert fb.lib.fb_lss_stepinfo_samples(nsteps, stride) == want == proto.samples_count(nsteps, stride) == fb.timeresp.samples(nsteps, stride)
    assert fb.lib.fb_lss_stepinfo_samples(0, 1) == -1 and fb.lib.fb_lss_stepinfo_samples(5, 0) == -1
    with pytest.raises(fb.FlightBatchError, match="at least 1"):
        fb.timeresp.samples(10, 0)


def test_the_kernels_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    names = {f"fbt::k_timeresp<{P}>" for P in (8, 16, 32)}
    assert {k for k in ks if k.startswith("fbt::")} == names, sorted(k for k in ks if k.startswith("fbt::"))
    for name in names:
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] <= 160 * 1024, (name, ks[name])
        assert ks[name]["lds"] == 512, (name, ks[name])      # (the doc's table: one double per lane of the wave)
        assert not re.search(r"\bk_step_", name) and "k_lss_" not in name and "k_lqr" not in name


def test_refusals_that_need_no_device(fb):
    info, status = np.empty(9), np.empty(1, dtype=np.int32)
    ch = np.zeros(1, dtype=np.int32)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = fb.lib.fb_lss_stepinfo(None, pi(ch), pi(ch), 1, 1.0, 0.01, None, None, None, 1, None, pd(info), pi(status))
    assert rc != 0 and b"null handle" in fb.lib.fb_last_error()


# ---- the notebook's stored tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["rk4", "exact"])
@pytest.mark.parametrize("which", ["velocity_loop", "position_loop"])
def test_prototype_reproduces_the_notebooks_table(which, side, capsys):
    A, b, c, d = proto.notebook_loops_from_golden()[0 if which == "velocity_loop" else 1]
    t = proto.stored_tables()[which]
    assert (t["t_sim"], t["dt"]) == ((5.0, 0.0062) if which == "velocity_loop" else (10.0, 0.005))
    N = int(round(t["t_sim"] / t["dt"]))
    fn = proto.samples_rk4 if side == "rk4" else proto.samples_exact
    y = fn(A[None], b[None], c[None], np.array([d]), N, t["dt"])[:, 0]
    info, status, (ipeak, iset, ilo, ihi) = proto.stepinfo(y, t["dt"])
    lines = proto.show(info)
    m = proto.margins(y)
    with capsys.disabled():
        print(f"\n[stepinfo prototype, {which}, {side}] N {N}: " + "; ".join(s.split(":")[0] + " " + s.split(":")[1].strip() for s in lines)
              + f"; indices peak {ipeak} settle {iset} rise {ilo}..{ihi}; smallest margin {min(m.values()):.2e}", end="")
    assert status == 0
    proto.assert_matches_table(lines, which)
    if which == "position_loop":
        assert ipeak == N and abs(info[4] - 9.995) <= 0.005 + 1e-12      # (monotone to its end: the peak is the last sample)
    assert min(m[k] for k in ("rise_lo", "rise_hi", "settling")) >= 8e-6      # the printed digits do not hinge on rounding


def test_show_prints_a_failed_pair(fb):
    nan = np.nan
    one = lambda v: np.array([[v]])
    si = fb.StepInfo(one(0.0), one(0.0), one(0.0), one(0.0), one(0.0), one(nan), one(nan), one(nan), one(nan), status=np.array([[2]], np.int32), dt=0.01)
    lines = si.show(0, 0).split("\n")
    assert lines == proto.show(np.array([0.0, 0.0, 0.0, 0.0, 0.0, nan, nan, nan, nan]))
    assert lines[5] == "Overshoot:           NaN %" and lines[8] == "Rise time:         NaN s" and not si.ok[0, 0]
    vals = np.array([0.0, 1.0234, 1.0234, 1.1652, 1.2834, 13.9, 27.452, 3.8936, 0.3596])
    si = fb.StepInfo(*[one(v) for v in vals], status=np.zeros((1, 1), np.int32), dt=0.0062)
    assert si.show().split("\n") == proto.show(vals) == proto.stored_tables()["velocity_loop"]["lines"] and si.ok.all()


# ---- the GPU tests' systems: the prototype against the exact side, and the condition on the inputs ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(nx):
    A, B, Cm, D = proto.plants(nx)
    P = proto.pairs(A, B, Cm, D, proto.CHANNELS)
    N = int(round(proto.T_SIM / proto.DT))
    return P, proto.samples_rk4(*P, N, proto.DT), proto.samples_exact(*P, N, proto.DT)


def _variants(P, Y):
    """the (y0_in, yf_in, opts) each GPU test runs the pairs with (tests/test_gpu_timeresp.py builds them through the same helper)"""
    return proto.gpu_variants(P, Y)


@pytest.mark.parametrize("nx", proto.NX_ALL + (12,))
def test_prototype_against_the_exact_side_and_the_margins_of_the_gpu_cases(nx, capsys):
    P, Y, Ye = _case(nx)
    dev = proto.sample_dev(Y, Ye)
    worst = {}
    for name, (y0_in, yf_in, opts) in _variants(P, Y).items():
        info, status = proto.stepinfo_batch(Y, proto.DT, y0_in, yf_in, opts)
        info_e, status_e = proto.stepinfo_batch(Ye, proto.DT, y0_in, yf_in, opts)
        assert (status == 0).all() and (status_e == 0).all(), name
        assert np.array_equal(info[[4, 7, 8]], info_e[[4, 7, 8]], equal_nan=True), name      # the same indices from either side
        ms = [proto.margins(Y[:, p], None if y0_in is None else y0_in[p], None if yf_in is None else yf_in[p], opts) for p in range(Y.shape[1])]
        ms += [proto.margins(Ye[:, p], None if y0_in is None else y0_in[p], None if yf_in is None else yf_in[p], opts) for p in range(Y.shape[1])]
        worst[name] = min(min(m.values()) for m in ms)
    with capsys.disabled():
        print(f"\n[stepinfo prototype vs exact] nx {nx:2d} x {Y.shape[1]} pairs, N {Y.shape[0] - 1}: samples {dev.max():.2e} of max|y|; smallest margin "
              + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()), end="")
    assert dev.max() <= 1e-10          # RK4 at |lambda| dt <~ 1e-2: truncation (|lambda| dt)^4 / 120 per unit time, far below this
    assert min(worst.values()) >= MARGIN_MIN, worst


def test_margins_of_the_failure_case(capsys):
    sysm, ch, yf = proto.failure_case()
    P = proto.pairs(*sysm, ch)
    N = int(round(proto.T_SIM / proto.DT))
    Y = proto.samples_rk4(*P, N, proto.DT)
    info, status = proto.stepinfo_batch(Y, proto.DT, None, yf.reshape(-1))
    assert sorted(np.flatnonzero(status == proto.DIVERGED)) == [2, 9, 16] and list(np.flatnonzero(status == proto.FLAT)) == [11]
    assert status[5] == 0 and np.isnan(info[8, 5]) and np.isnan(info[8]).sum() == 5
    worst = min(min(proto.margins(Y[:, p], None, yf.reshape(-1)[p]).values()) for p in np.flatnonzero(status == 0))
    with capsys.disabled():
        print(f"\n[stepinfo prototype, failure case] smallest margin over the {int((status == 0).sum())} healthy pairs {worst:.2e}", end="")
    assert worst >= MARGIN_MIN
