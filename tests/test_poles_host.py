"""Poles on the device, host side (no GPU compute): fb_lss_poles is declared, exported, bound and wrapped; fbe::k_poles<8 | 16 | 32> are in
the library with 0 B of scratch and the LDS docs/design/linearize.md tabulates; the numpy restatement of the kernel's algorithm
(tests/poles_prototype.py) agrees with LAPACK, and LAPACK with itself, on the systems the GPU tests use — the preconditions that make
np.linalg.eigvals their yardstick; balancing is what the badly scaled case needs; the exact cases come out exactly; the prototype and
dampreport reproduce the two tables the reference's robot2d design notebook stores."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import poles_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    assert "fb_lss_poles" in declared
    assert re.search(r"\bT fb_lss_poles\b", out)
    assert "fb_lss_poles" in fb.EXPORTED and len(fb.lib.fb_lss_poles.argtypes) == 5
    assert "(:fb_lss_poles, lib)" in shim and re.search(r"^function poles\(w::LinearWorld\)", shim, flags=re.M)
    assert (fb.K["FB_POLES_NOT_CONVERGED"], fb.K["FB_POLES_NOT_FINITE"], fb.K["FB_POLES_NX_MAX"]) == (1, 2, 32)
    assert (proto.NOT_CONVERGED, proto.NOT_FINITE, proto.NX_MAX) == (1, 2, 32)
    import importlib
    P = importlib.import_module("flightbatch.poles")     # (the package's attribute `poles` is the verb)
    assert (P.NOT_CONVERGED, P.NOT_FINITE, P.NX_MAX) == (1, 2, 32)
    for name in ("poles", "dampreport", "PolesResult"):
        assert hasattr(fb, name)
    assert fb.lib.fb_lss_poles(None, None, None, None, None) != 0 and b"null handle" in fb.lib.fb_last_error()


def test_the_kernels_are_in_the_library(tmp_path_factory):
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    lds = {f"fbe::k_poles<{P}>": (64 // P) * P * (P + 1) * 8 for P in (8, 16, 32)}
    assert lds == {"fbe::k_poles<8>": 4608, "fbe::k_poles<16>": 8704, "fbe::k_poles<32>": 16896}     # (the doc's table)
    assert {k for k in ks if k.startswith("fbe::")} == set(lds), sorted(k for k in ks if k.startswith("fbe::"))
    for name, want in lds.items():
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == want, (name, ks[name])


@functools.lru_cache(maxsize=None)
def _reference(nx):
    A = proto.systems(nx)
    lam, iters, status = proto.poles_batch(A)
    mu = np.array([np.linalg.eigvals(a) for a in A])
    return A, lam, iters, status, mu


@pytest.mark.parametrize("nx", proto.NX_ALL)
def test_prototype_and_lapack_preconditions(nx, capsys):
    A, lam, iters, status, mu = _reference(nx)
    d_proto = proto.batch_dev(lam, mu)
    d_self = proto.batch_dev([np.linalg.eigvals(a.T) for a in A], mu)
    with capsys.disabled():
        print(f"\n[poles prototype vs LAPACK] nx {nx:2d} x {len(A)}: {d_proto:.2e}; LAPACK on A vs on A' {d_self:.2e}; "
              f"sweeps {iters.min()} / {int(np.median(iters))} / {iters.max()}", end="")
    assert (status == 0).all()
    assert d_proto <= 1e-12 and d_self <= 1e-12
    assert (d_proto == 0.0) if nx == 1 else True
    assert all(proto.sort_rule_holds(l) for l in lam)
    assert (iters <= 30 * nx).all()


def test_balancing_is_what_the_badly_scaled_case_needs(capsys):
    A, As = proto.badly_scaled()
    mu = np.linalg.eigvals(A)
    lam, _, st = proto.poles(As)
    raw, _, st_raw = proto.poles(As, balancing=False)
    d, d_raw = proto.match_dev(lam, mu), proto.match_dev(raw, mu)
    with capsys.disabled():
        print(f"\n[poles prototype, badly scaled] with balancing {d:.2e}, without {d_raw:.2e}", end="")
    assert st == 0 and st_raw == 0
    assert d <= 1e-12
    assert d_raw >= 1e-10


def test_balancing_is_an_exact_similarity_by_powers_of_two():
    _, As = proto.badly_scaled()
    B = proto.balance(As.copy(), 16)
    ratio = B / As
    m, e = np.frexp(ratio)
    assert (m == 0.5).all()                                   # every entry scaled by a power of two
    d = ratio[:, 0]                                           # D A inv(D): ratio[i, j] = d_i / d_j
    assert np.array_equal(ratio, d[:, None] / d[None, :])
    assert np.array_equal(np.diag(B), np.diag(As))


def test_exact_cases():
    for A, want in proto.exact_cases():
        lam, sweeps, st = proto.poles(A)
        assert st == 0
        assert np.array_equal(lam.real, want.real) and np.array_equal(lam.imag, want.imag), (A, lam, want)
    lam, sweeps, st = proto.poles(np.array([[1.0, np.nan], [0.0, 1.0]]))
    assert st == proto.NOT_FINITE and sweeps == 0 and np.isnan(lam).all()
    lam, sweeps, st = proto.poles(np.array([[1.0, 0.0], [np.inf, 1.0]]))
    assert st == proto.NOT_FINITE and sweeps == 0 and np.isnan(lam).all()


# ---- the notebook's stored tables (the fixtures and their tolerances: tests/poles_prototype.py) --------------------------------------------
@pytest.mark.parametrize("which", ["open_loop", "velocity_loop"])
def test_prototype_reproduces_the_notebooks_table(fb, which):
    A = proto.notebook_systems()[0 if which == "open_loop" else 1]
    lam, _, st = proto.poles(A)
    assert st == 0
    proto.assert_matches_table(lam, which)
    header, lines, _ = proto.table_rows(which)
    assert proto.report_with_zero_snapped(fb, lam) == header + lines


def test_dampreport_prints_a_complex_pair_and_a_failed_system(fb):
    res = fb.PolesResult(poles=np.array([[-0.5 - 2.0j, -0.5 + 2.0j], [np.nan + 1j * np.nan] * 2]), iters=np.zeros(2, np.int32),
                         status=np.array([0, 2], np.int32))
    rows = fb.dampreport(res, 0).split("\n")[3:]
    assert rows[0].startswith("| -0.5    - 2     im |") and rows[1].startswith("| -0.5    + 2     im |")
    assert all(len(r) == len(rows[0]) for r in rows)
    assert "0.243" in rows[0] and "2.06" in rows[0]           # zeta = 0.5 / |pole|, wn = |pole|
    assert np.array_equal(res.stable, [True, False])
    assert "NaN" in fb.dampreport(res, 1)
