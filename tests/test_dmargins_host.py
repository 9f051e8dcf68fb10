"""Sampled loops on the device, host side (no GPU compute): fb_lss_set_sampled, fb_lss_dfreqresp, fb_lss_dmargins and fb_lss_dpoles are
declared, exported, bound and wrapped; the kernels of namespace fbw are exactly the six instances, each with 0 B of scratch and the LDS
its layout gives; the refusals that need no device; and the numpy restatement of the kernels (tests/dmargins_prototype.py) is held to the
exact side (numpy.linalg.solve for L, scipy.optimize.brentq on θ inside the same grid brackets, closed forms where they exist) over the
GPU tests' cases, which are checked to be fair on the exact side: every grid value has |Im L_k| >= 1e-9 |L_k| and | |L_k|² - 1 | >= 1e-9,
every accepted phase crossing has -Re L* >= 1e-3, and the prototype's worst deviation is <= 1e-9 — the conditions under which
tests/test_gpu_dmargins.py may hold the device to ten times the prototype's deviation. The largest number of halvings a bracket takes
over all these cases is printed: the kernel's cap is that figure plus 10."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dmargins_prototype as proto
import margins_prototype as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERBS = {"fb_lss_set_sampled": 2, "fb_lss_dfreqresp": 7, "fb_lss_dmargins": 10, "fb_lss_dpoles": 5}


def test_the_symbols_are_declared_exported_bound_and_wrapped(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h"), encoding="utf-8").read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    for name, nargs in VERBS.items():
        assert name in declared and re.search(rf"\bT {name}\b", out), name
        assert name in fb.EXPORTED and len(getattr(fb.lib, name).argtypes) == nargs, name
        assert f"(:{name}, lib)" in shim, name
    assert set(fb.EXPORTED) == declared          # the binding's table is the header
    for fn in ("set_sampled!", "dfreqresp", "dmargins", "dpoles"):
        assert re.search(rf"^(function )?{re.escape(fn)}\(w::LinearWorld", shim, flags=re.M), fn
    assert list(inspect.signature(fb.dmargins).parameters) == ["world", "u", "y", "w", "gain", "all"]
    assert list(inspect.signature(fb.dfreqresp).parameters) == ["world", "u", "y", "w"]
    assert "Ts" in inspect.signature(fb.LinearWorld.__init__).parameters
    assert inspect.signature(fb.dmargins).return_annotation in (fb.MarginsResult, "MarginsResult")
    for name in ("poles", "s", "wn", "zeta", "tau", "stable", "status", "iters"):
        assert hasattr(fb.DPolesResult, name) or name in fb.DPolesResult.__dataclass_fields__, name
    assert callable(fb.dpoles) and callable(fb.ddampreport)
    assert (proto.NOT_FINITE, proto.SINGULAR, proto.TRUNCATED, proto.KMAX) == tuple(
        fb.K[k] for k in ("FB_MARGINS_NOT_FINITE", "FB_MARGINS_SINGULAR", "FB_MARGINS_TRUNCATED", "FB_MARGINS_KMAX"))


def test_the_kernels_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    # per group of P lanes: the scaled pivot row with its right-hand side (P + 1 complex), the solution (P complex) and c (P): 5 P + 2
    # doubles; the margins add 32 bracket words; 64 / P groups to a one-wave workgroup
    want = {f"fbw::k_lss_dfreqresp<{P}>": (5 * P + 2) * (64 // P) * 8 for P in (8, 16, 32)}
    want.update({f"fbw::k_lss_dmargins<{P}>": (5 * P + 34) * (64 // P) * 8 for P in (8, 16, 32)})
    assert {k for k in ks if k.startswith("fbw::")} == set(want), sorted(k for k in ks if k.startswith("fbw::"))
    for name, lds in want.items():
        print(name, ks[name])
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == lds, (name, ks[name])
        assert "k_step_" not in name


def test_the_cap_in_the_kernel_is_the_prototypes():
    text = open(os.path.join(ROOT, "flight.jl_amd", "csrc", "dfreq_kernels.hpp"), encoding="utf-8").read()
    assert int(re.search(r"constexpr int DM_ITERS = (\d+);", text).group(1)) == proto.ITERS == proto.OBSERVED + 10
    assert re.search(rf"\b{proto.OBSERVED}\b", text.split("constexpr int DM_ITERS")[0].rsplit("\n\n", 1)[-1])      # both numbers in the comment


def test_refusals_that_need_no_device(fb):
    w = np.logspace(-1, 1, 9)
    sel, counts, status = np.empty(10), np.empty(2, dtype=np.int32), np.empty(1, dtype=np.int32)
    re_, im_ = np.empty(9), np.empty(9)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    calls = {"fb_lss_set_sampled": lambda: fb.lib.fb_lss_set_sampled(None, 0.02),
             "fb_lss_dfreqresp": lambda: fb.lib.fb_lss_dfreqresp(None, 0, 0, w.ctypes.data_as(D), w.size, re_.ctypes.data_as(D), im_.ctypes.data_as(D)),
             "fb_lss_dmargins": lambda: fb.lib.fb_lss_dmargins(None, 0, 0, w.ctypes.data_as(D), w.size, None, sel.ctypes.data_as(D), counts.ctypes.data_as(I),
                                                               None, status.ctypes.data_as(I)),
             "fb_lss_dpoles": lambda: fb.lib.fb_lss_dpoles(None, re_.ctypes.data_as(D), im_.ctypes.data_as(D), None, status.ctypes.data_as(I))}
    for name, call in calls.items():
        assert call() != 0
        err = fb.lib.fb_last_error()
        assert b"null handle" in err and name.encode() in err, err
    for verb in (fb.dmargins, fb.dpoles, lambda x: fb.dfreqresp(x, 0, 0, w)):
        with pytest.raises(fb.FlightBatchError, match="LinearWorld"):
            verb(object())


def test_the_default_grid_ends_at_the_nyquist_frequency(fb):
    for Ts in (0.02, 0.05, 1.0 / 3.0, 0.7, 1e-3, 17.0):
        w = fb.default_dgrid(Ts)
        assert w.size == 321 and (np.diff(w * Ts) > 0.0).all() and w[-1] * Ts <= np.pi and abs(w[-1] * Ts / np.pi - 1.0) <= 4e-16
        assert abs(w[0] / (1e-4 * np.pi / Ts) - 1.0) <= 1e-12


# ---- the prototype against the exact side over the GPU tests' cases, and the cases themselves ---------------------------------------------------
def _zoh_embedded(Ts, nx=9, seed=9):
    rng = np.random.default_rng(seed)
    return [(proto.zoh(mp.embed(proto.cube(K), nx, rng), Ts), proto.w_zoh(Ts), Ts, 1.0) for K in mp.K_CLOSED]


CASES = {f"K / (z (z - 1)) in nx = {nx}": (lambda nx=nx: [(s, proto.W_CLOSED, proto.TS_CLOSED, 1.0) for s, _ in proto.closed_systems(nx)]) for nx in proto.NX_CLOSED}
CASES.update({f"the hold of K / (s + 1)³ at Ts = {Ts:g}": (lambda Ts=Ts: [(proto.zoh(proto.cube(K), Ts), proto.w_zoh(Ts), Ts, 1.0) for K in mp.K_CLOSED]) for Ts in proto.TS_ZOH})
CASES.update({f"the c2d chain in nx = 9 at Ts = {Ts:g}": (lambda Ts=Ts: _zoh_embedded(Ts)) for Ts in (0.05, 0.5)})
CASES["0 to 3 crossings"] = lambda: [(proto.zoh(s, proto.TS_WORK), proto.W_WORK, proto.TS_WORK, 1.0) for _, s in proto.work_systems()[:10]]
CASES.update({f"crossings in the first and last of {nw - 1} intervals": (lambda nw=nw: [(proto.delay_integrator(K), proto.edge_grid(K, nw), proto.TS_CLOSED, 1.0) for K in proto.K_DELAY])
              for nw in (65, 66, 130)})
CASES["six lightly damped modes"] = lambda: [(proto.zoh(proto.modes(), proto.TS_MODES), proto.W_MODES, proto.TS_MODES, 1.0)]
CASES["gain 0.6 and per system"] = lambda: [(proto.closed_systems(9)[1][0], proto.W_CLOSED, proto.TS_CLOSED, g) for g in (0.6, 1.0, 2.0, 0.3, 1.5)]
CASES["K on both sides of 1"] = lambda: [(proto.delay_integrator(K), proto.W_CLOSED, proto.TS_CLOSED, 1.0) for K in proto.K_STABILITY]


@functools.lru_cache(maxsize=None)
def _held(label):
    """(worst deviation, fairness, largest halving count, results) of the prototype over a case list"""
    worst, fair, results = 0.0, [np.inf, np.inf, np.inf], []
    before, proto.HALVINGS[0] = proto.HALVINGS[0], 0
    for s, w, Ts, gain in CASES[label]():
        got = proto.margins(*s, w, Ts, gain)
        ex, L = proto.exact(*s, w, Ts, gain)
        worst = max(worst, proto.deviation(got, ex))
        fair = [min(a, b) for a, b in zip(fair, proto.fairness(L, ex))]
        results.append((got, ex, L))
    halvings, proto.HALVINGS[0] = proto.HALVINGS[0], max(before, proto.HALVINGS[0])
    return worst, fair, halvings, results


@pytest.mark.parametrize("label", list(CASES))
def test_the_prototype_holds_to_the_exact_side(label, capsys):
    worst, fair, halvings, results = _held(label)
    with capsys.disabled():
        print(f"\n[dmargins prototype vs exact] {label}, {len(results)} systems: worst deviation {worst:.2e}; min |Im L_k| / |L_k| {fair[0]:.1e}, "
              f"min ||L_k|² - 1| {fair[1]:.1e}, min accepted -Re L* {fair[2]:.1e}; at most {halvings} halvings", end="")
    assert fair[0] >= proto.FAIR_GRID and fair[1] >= proto.FAIR_GRID and fair[2] >= proto.FAIR_GM
    assert worst <= proto.PROTO_MAX
    assert halvings < proto.ITERS


def test_the_largest_halving_count_is_below_the_cap(capsys):
    most = max(_held(label)[2] for label in CASES)
    with capsys.disabled():
        print(f"\n[dmargins prototype] the largest halving count over {len(CASES)} case lists: {most}; the cap is {proto.ITERS}", end="")
    assert most <= proto.OBSERVED and proto.ITERS == proto.OBSERVED + 10


@pytest.mark.parametrize("nx", proto.NX_CLOSED)
def test_closed_forms(nx, capsys):
    results = _held(f"K / (z (z - 1)) in nx = {nx}")[3]
    worst = 0.0
    for (_, K), (got, ex, L) in zip(proto.closed_systems(nx), results):
        gm, wpc, pm, wgc = proto.delay_closed_form(K, proto.TS_CLOSED)
        for sel, counts in (got[:2], ex[:2]):
            assert tuple(counts) == (1, 1)
            worst = max(worst, abs(sel[0] / gm - 1.0), abs(sel[1] / wpc - 1.0), abs(sel[2] - pm) / 180.0, abs(sel[3] / wgc - 1.0))
    with capsys.disabled():
        print(f"\n[dmargins prototype] K / (z (z - 1)) in nx = {nx}: closed forms {worst:.2e}", end="")
    assert worst <= 1e-11          # (the trial met them to 5e-15 up to nx = 16 and 5e-12 at nx = 32)


def _one_bracket_each(L):
    ph, ga = proto.brackets(L)
    assert len(ph) == 1 and len(ga) == 1, (ph, ga)
    assert (np.abs(L.imag) / np.abs(L)).min() >= 1e-2 and np.abs(np.abs(L) ** 2 - 1.0).min() >= 1e-2


def test_the_33_point_grids_have_one_bracket_of_each_kind():
    for K in proto.K_DELAY:
        _one_bracket_each(proto.exact(*proto.delay_integrator(K), proto.W_CLOSED, proto.TS_CLOSED)[1])
    for Ts in proto.TS_ZOH:
        for K in mp.K_CLOSED:
            _one_bracket_each(proto.exact(*proto.zoh(proto.cube(K), Ts), proto.w_zoh(Ts), Ts)[1])


def test_the_hold_costs_phase_margin():
    """the rule of thumb the example prints: a zero-order hold at Ts takes about ω_gc Ts / 2 of phase margin"""
    for K in mp.K_CLOSED:
        gm, wpc, pm, wgc = mp.cube_closed_form(K)
        sel = proto.margins(*proto.zoh(proto.cube(K), 0.05), proto.w_zoh(0.05), 0.05)[0]
        assert abs((pm - sel[2]) - np.degrees(wgc * 0.05 / 2.0)) <= 0.05 and sel[0] < gm


def test_unequal_work_batch():
    results = _held("0 to 3 crossings")[3]
    names = [k for k, _ in proto.work_systems()[:5]]
    by = dict(zip(names, (tuple(r[0][1]) for r in results[:5])))
    assert len(set(by.values())) >= 4 and {sum(v) for v in by.values()} >= {0, 1, 2, 3}, by          # 0, 1, 2 and 3 crossings
    for got, ex, _ in results:
        assert tuple(got[1]) == tuple(ex[1])


@pytest.mark.parametrize("nw", [65, 66, 130])
def test_grid_edges(nw):
    for _, _, L in _held(f"crossings in the first and last of {nw - 1} intervals")[3]:
        ph, ga = proto.brackets(L)
        assert ph.tolist() == [nw - 2] and ga.tolist() == [0]


def test_more_crossings_than_are_kept():
    (got, ex, L), = _held("six lightly damped modes")[3]
    sel, counts, allv, status = got
    assert len(proto.brackets(L)[1]) > proto.KMAX
    assert status == proto.TRUNCATED and tuple(counts) == (0, proto.KMAX) and (np.diff(allv[3]) > 0.0).all()


def test_gain_scales_the_margin():
    res = _held("gain 0.6 and per system")[3]
    k, one = res[0][0][0], res[1][0][0]
    assert abs(k[0] / (one[0] / 0.6) - 1.0) <= 1e-12 and abs(k[1] / one[1] - 1.0) <= 1e-12


def test_margins_and_stability_agree():
    """the closed loop of K / (z (z - 1)) is z² - z + K: stable exactly for 0 < K < 1, where the gain margin 1 / K exceeds 1"""
    for (got, _, _), K in zip(_held("K on both sides of 1")[3], proto.K_STABILITY):
        Phi, g, c, d = proto.delay_integrator(K)
        stable = np.abs(np.linalg.eigvals(Phi - np.outer(g, c))).max() < 1.0
        assert (got[0][0] > 1.0) == stable == (K < 1.0), K


def test_bad_inputs():
    Phi, g, c, d = proto.delay_integrator(0.5)
    w, Ts = proto.W_CLOSED[::4], proto.TS_CLOSED
    bad = Phi.copy(); bad[1, 0] = np.nan
    assert proto.margins(bad, g, c, d, w, Ts)[3] == proto.NOT_FINITE and proto.margins(Phi, g, c, d, w, Ts, np.nan)[3] == proto.NOT_FINITE
    assert proto.margins(Phi, 1e308 * g, 1e308 * c, d, w, Ts)[3] == proto.SINGULAR          # L overflows
    assert proto.margins(Phi, g, c, d, w, Ts)[3] == 0
    # a pole hit exactly on the circle: the integrator's at z = 1 and a pole at z = -1, the points handed over directly (through the ABI
    # neither can be arranged: w > 0, and sin π is not 0 in double)
    cs, sn = proto.circle(w, Ts)
    for z, P in ((1.0, Phi), (-1.0, np.array([[-1.0, 0.0], [1.0, 0.0]]))):
        cs1, sn1 = cs.copy(), sn.copy()
        cs1[3], sn1[3] = z, 0.0
        sel, counts, allv, status = proto.margins_z(P, g, c, d, cs1, sn1, w, Ts)
        assert status == proto.SINGULAR and np.isnan(sel).all() and np.isnan(allv).all() and tuple(counts) == (0, 0)
        assert proto.margins_z(P, g, c, d, cs, sn, w, Ts)[3] == 0


def test_dfreqresp_restated():
    rng = np.random.default_rng(4)
    for nx in (2, 9, 17):
        s = proto.closed_systems(nx)[0][0]
        got = proto.dfreqresp(*s, proto.W_CLOSED, proto.TS_CLOSED)
        want = np.array([proto.exact_response(*s, np.exp(1j * w * proto.TS_CLOSED)) for w in proto.W_CLOSED])
        assert np.abs(got / want - 1.0).max() <= 1e-11
