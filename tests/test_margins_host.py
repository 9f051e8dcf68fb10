"""Margins on the device, host side (no GPU compute): fb_lss_margins is declared, exported, bound and wrapped; fbn::k_lss_margins<8 | 16 | 32>
are in the library with 0 B of scratch and are no stepping kernels; the refusals that need no device; and the numpy restatement of the
kernel (tests/margins_prototype.py) is held to the exact side (numpy.linalg.solve for L, scipy.optimize.brentq inside the same grid
brackets, closed forms where they exist) over the GPU tests' cases, which are checked to be fair: every grid value has |Im L_k| >= 1e-9 |L_k|
and | |L_k|² - 1 | >= 1e-9, every accepted phase crossing has -Re L* >= 1e-3, and the prototype's worst deviation is <= 1e-9 — the
conditions under which tests/test_gpu_margins.py may hold the device to ten times the prototype's deviation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import margins_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_exported_bound_and_wrapped(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h"), encoding="utf-8").read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    assert "fb_lss_margins" in declared and re.search(r"\bT fb_lss_margins\b", out)
    assert "fb_lss_margins" in fb.EXPORTED and len(fb.lib.fb_lss_margins.argtypes) == 10
    assert "(:fb_lss_margins, lib)" in shim and re.search(r"^function margins\(w::LinearWorld", shim, flags=re.M)
    got = tuple(fb.K[k] for k in ("FB_MARGINS_NOT_FINITE", "FB_MARGINS_SINGULAR", "FB_MARGINS_TRUNCATED", "FB_MARGINS_KMAX", "FB_MARGINS_NX_MAX"))
    assert got == (1, 2, 4, 8, 32) == (proto.NOT_FINITE, proto.SINGULAR, proto.TRUNCATED, proto.KMAX, proto.NX_MAX)
    import inspect
    assert callable(fb.margins) and hasattr(fb, "MarginsResult")
    assert list(inspect.signature(fb.margins).parameters) == ["world", "u", "y", "w", "gain", "all"]
    for name in ("gm", "gm_db", "wpc", "pm", "wgc", "ms", "wms", "npc", "ngc", "status", "ok", "gm_all", "wpc_all", "pm_all", "wgc_all", "show"):
        assert hasattr(fb.MarginsResult, name) or name in fb.MarginsResult.__dataclass_fields__, name


def test_the_kernels_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    want = {f"fbn::k_lss_margins<{P}>": (5 * P + 34) * (64 // P) * 8 for P in (8, 16, 32)}   # pivot row, solution, c and 32 bracket words per group
    assert {k for k in ks if k.startswith("fbn::")} == set(want), sorted(k for k in ks if k.startswith("fbn::"))
    for name, lds in want.items():
        print(name, ks[name])
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == lds, (name, ks[name])
        assert "k_step_" not in name


def test_refusals_that_need_no_device(fb):
    w = np.logspace(-1, 1, 9)
    sel, counts, status = np.empty(10), np.empty(2, dtype=np.int32), np.empty(1, dtype=np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = fb.lib.fb_lss_margins(None, 0, 0, w.ctypes.data_as(D), w.size, None, sel.ctypes.data_as(D), counts.ctypes.data_as(I), None, status.ctypes.data_as(I))
    assert rc != 0 and b"null handle" in fb.lib.fb_last_error()
    with pytest.raises(fb.FlightBatchError, match="LinearWorld"):
        fb.margins(object())


# ---- the prototype against the exact side over the GPU tests' cases, and the cases themselves ---------------------------------------------------
def _hold(label, cases, capsys):
    """cases: [(system, w, gain)]; the fairness conditions on the exact side and the prototype's deviation"""
    worst, fair = 0.0, [np.inf, np.inf, np.inf]
    for s, w, gain in cases:
        got = proto.margins(*s, w, gain)
        ex, L = proto.exact(*s, w, gain)
        worst = max(worst, proto.deviation(got, ex))
        fair = [min(a, b) for a, b in zip(fair, proto.fairness(L, ex))]
    with capsys.disabled():
        print(f"\n[margins prototype vs exact] {label}, {len(cases)} systems: worst deviation {worst:.2e}; min |Im L_k| / |L_k| {fair[0]:.1e}, "
              f"min ||L_k|² - 1| {fair[1]:.1e}, min accepted -Re L* {fair[2]:.1e}", end="")
    assert fair[0] >= proto.FAIR_GRID and fair[1] >= proto.FAIR_GRID and fair[2] >= proto.FAIR_GM
    assert worst <= proto.PROTO_MAX
    return worst


@pytest.mark.parametrize("nx", proto.NX_CLOSED)
def test_closed_forms(nx, capsys):
    systems = proto.closed_systems(nx)
    _hold(f"K / (s + 1)³ in nx = {nx}", [(s, proto.W_CLOSED, 1.0) for s, _ in systems], capsys)
    worst = 0.0
    for s, K in systems:
        for side in (proto.margins(*s, proto.W_CLOSED), proto.exact(*s, proto.W_CLOSED)[0]):
            sel, counts = side[0], side[1]
            gm, wpc, pm, wgc = proto.cube_closed_form(K)
            assert tuple(counts) == (1, 1)
            worst = max(worst, abs(sel[0] / gm - 1.0), abs(sel[1] / wpc - 1.0), abs(sel[2] - pm) / 180.0, abs(sel[3] / wgc - 1.0))
    with capsys.disabled():
        print(f"; closed forms {worst:.2e}", end="")
    assert worst <= 1e-11          # (a plain random similarity met them to 3e-12 at nx = 32)


def test_small_and_degenerate_plants(capsys):
    w = np.logspace(-2.0, 2.0, 65)
    first = lambda K: proto.tf([K], [1.0, 1.0])
    integ = lambda K: proto.tf([K], [1.0, 1.0, 0.0])
    _hold("nx = 1 and 2", [(first(3.0), w, 1.0), (first(0.5), w, 1.0), (integ(3.0), w, 1.0), (integ(0.4), w, 1.0)], capsys)
    sel, counts, _, status = proto.margins(*first(3.0), w)
    assert tuple(counts) == (0, 1) and sel[0] == np.inf and abs(sel[3] / np.sqrt(8.0) - 1.0) <= 1e-14
    assert abs(sel[2] - (180.0 - np.degrees(np.arctan(np.sqrt(8.0))))) <= 1e-12
    sel, counts, allv, status = proto.margins(*first(0.5), w)
    assert tuple(counts) == (0, 0) and status == 0 and sel[0] == sel[2] == np.inf and np.isnan(sel[[1, 3]]).all() and np.isnan(allv).all()
    assert sel[9] == w[-1]          # |1 + L| falls with ω: the grid's last point, which has no interval of its own at 65 frequencies
    sel, counts, _, status = proto.margins(*integ(3.0), w)
    assert tuple(counts) == (0, 1) and sel[0] == np.inf and np.isnan(sel[1])


def test_unequal_work_batch(capsys):
    systems = proto.work_systems()
    _hold(f"0 to 3 crossings in nx = {proto.NX_WORK}", [(s, proto.W_WORK, 1.0) for _, s in systems[:10]], capsys)
    by = {name: proto.margins(*s, proto.W_WORK) for name, s in systems[:5]}
    assert [tuple(by[k][1]) for k in ("none", "one", "two", "three", "first-order")] == [(0, 0), (0, 1), (1, 1), (2, 1), (0, 1)]
    assert by["three"][0][0] < 1.0      # the conditionally stable loop: the selected gain margin is a gain reduction


@pytest.mark.parametrize("nw", [65, 70, 130])
def test_grid_edges(nw, capsys):
    cases = [(proto.cube(K), proto.edge_grid(K, nw), 1.0) for K in proto.K_CLOSED]
    _hold(f"crossings in the first and last of {nw - 1} intervals", cases, capsys)
    for s, w, _ in cases:
        ph, ga = proto.brackets(proto.exact(*s, w)[1])
        assert ph.tolist() == [nw - 2] and ga.tolist() == [0]


def test_more_crossings_than_are_kept(capsys):
    s = proto.modes()
    _hold("six lightly damped modes", [(s, proto.W_MODES, 1.0)], capsys)
    sel, counts, allv, status = proto.margins(*s, proto.W_MODES)
    assert len(proto.brackets(proto.exact(*s, proto.W_MODES)[1])[1]) > proto.KMAX
    assert status == proto.TRUNCATED and tuple(counts) == (0, proto.KMAX) and (np.diff(allv[3]) > 0.0).all()


def test_gain_scales_the_margin(capsys):
    s = proto.closed_systems(9)[1][0]
    _hold("gain 0.6", [(s, proto.W_CLOSED, 0.6)], capsys)
    one, k = proto.margins(*s, proto.W_CLOSED)[0], proto.margins(*s, proto.W_CLOSED, 0.6)[0]
    assert abs(k[0] / (one[0] / 0.6) - 1.0) <= 1e-12 and abs(k[1] / one[1] - 1.0) <= 1e-12


def test_bad_inputs():
    A, b, c, d = proto.tf([3.0], [1.0, 1.0, 0.0])
    w = np.array([0.25, 0.5, 1.0, 2.0, 4.0])
    bad = A.copy(); bad[1, 0] = np.nan
    assert proto.margins(bad, b, c, d, w)[3] == proto.NOT_FINITE and proto.margins(A, b, c, d, w, np.nan)[3] == proto.NOT_FINITE
    sel, counts, allv, status = proto.margins(np.array([[0.0, 1.0], [-1.0, 0.0]]), b, c, d, w)      # jωI - A is singular at ω = 1 exactly
    assert status == proto.SINGULAR and np.isnan(sel).all() and np.isnan(allv).all() and tuple(counts) == (0, 0)
    assert proto.margins(A, b, c, d, w)[3] == 0
