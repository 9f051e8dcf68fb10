"""Closing sampled loops on the device, host side (no GPU compute): fb_lss_dconnect is declared, exported, bound and wrapped;
fbv::k_dconnect<8 | 16 | 32> are in the library with 0 B of scratch; the refusals that need no device; the numpy restatement
(tests/dconnect_prototype.py) on the generator of the GPU tests: status 0 everywhere, its float64 side within 1e-14 of its longdouble side
(the condition under which tests/test_gpu_dconnect.py's accuracy rule means what it says), and twelve ticks of the float64 result under
random inputs against a tick-by-tick simulation of the interconnection with explicit delay buffers, which does not use the formula.

The tick bound, 1e-11 of the largest output, is the floor tests/test_gpu_dconnect.py holds the device's stepping to. Reasoning: both sides
are float64; a tick is sums of at most 32 + 16 terms behind a solve with cond(E) <= 3, so one tick of either side is within about
48 x 3 x eps = 1.6e-14 of exact, twelve ticks of both within 4e-13 to first order; the rest is what powers of Phi' may amplify, relative
to the largest output of the run. An indexing error, a delayed read taken now or a buffer written a tick early is of order 1. Measured
(this generator): at most 8.3e-14 (20/2/4/1/38/1/10/5/2/39), between 3e-15 and 2.8e-14 on the other shapes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dconnect_prototype as proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK_BOUND = 1e-11


def test_the_symbol_is_declared_exported_and_bound(fb):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flightbatch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fb_[a-z_0-9]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", fb.LIB_PATH], capture_output=True, text=True).stdout
    shim = open(os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl"), encoding="utf-8").read()
    assert "fb_lss_dconnect" in declared and re.search(r"\bT fb_lss_dconnect\b", out)
    assert "fb_lss_dconnect" in fb.EXPORTED and len(fb.lib.fb_lss_dconnect.argtypes) == 15
    assert "(:fb_lss_dconnect, lib)" in shim and re.search(r"^function dconnect\(p::LinearWorld", shim, flags=re.M)
    assert fb.K["FB_DCONNECT_ND_MAX"] == 31 == proto.ND_MAX
    import importlib
    dc = importlib.import_module("flightbatch.dconnect")      # (the package attribute of that name is the verb)
    assert dc.ND_MAX == 31 and dc.DELAYED == "[k-1]"
    for name in ("dconnect", "dintegrator_world", "dpid_world", "dstate_feedback", "dseries", "dunity_feedback"):
        assert hasattr(fb, name) and getattr(fb, name) is getattr(dc, name)


def test_the_kernels_are_in_the_library(tmp_path_factory):
    """exactly the instances the dispatcher of fb_lss_dconnect can launch, with the resources the doc tabulates; fbc::k_connect as it was"""
    from support import library_kernels
    ks = library_kernels(tmp_path_factory)
    lds = {"fbv::k_dconnect<8>": 10240, "fbv::k_dconnect<16>": 14080, "fbv::k_dconnect<32>": 11392}
    assert {k for k in ks if k.startswith("fbv::")} == set(lds), sorted(k for k in ks if k.startswith("fbv::"))
    for name, want in lds.items():
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == want, (name, ks[name])
    assert {k for k in ks if k.startswith("fbc::")} == {"fbc::k_connect<8>", "fbc::k_connect<16>", "fbc::k_connect<32>"}


def test_the_shapes_put_the_extended_state_at_both_edges_of_every_group_size():
    sizes = {}
    for s in proto.SHAPES:
        nxp, nxc, nup, nuc, nyp, nyc, nd, nf, nw, ny = s
        assert 1 <= proto.nxe(s) <= 32 and nup + nuc <= 16 and nyp + nyc + nd <= 128 and 0 <= nd <= 31 and 1 <= nf <= 32 and 1 <= nw <= 8 and 1 <= ny <= 64
        assert nf <= nyp + nyc + nd and ny <= nyp + nyc + nd
        sizes.setdefault(proto.group(proto.nxe(s), nup + nuc), set()).add(proto.nxe(s))
    assert {2, 8} <= sizes[8] and {9, 16} <= sizes[16] and {17, 32} <= sizes[32], sizes
    assert sum(s[6] == 0 for s in proto.SHAPES) == 1


def test_refusals_that_need_no_device(fb):
    h = C.c_void_p(1)
    one = np.zeros(1, dtype=np.int32)
    g = np.ones(1)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = fb.lib.fb_lss_dconnect(None, None, pi(one), 1, pi(one), 1, pd(g), 0, pd(g), 0, 1, None, 0, None, C.byref(h))
    assert rc != 0 and b"fb_lss_dconnect" in fb.lib.fb_last_error() and b"null handle" in fb.lib.fb_last_error() and not h.value
    rc = fb.lib.fb_lss_dconnect(None, None, pi(one), 1, pi(one), 1, pd(g), 0, pd(g), 0, 1, None, 0, None, None)
    assert rc != 0 and b"fb_lss_dconnect" in fb.lib.fb_last_error() and b"out is null" in fb.lib.fb_last_error()


# ---- the prototype against itself --------------------------------------------------------------------------------------------------------------
def test_extend_with_no_delay_is_the_stacked_model_and_the_prototype_is_connects():
    import connect_prototype as cp
    shape = proto.SHAPES[-1]
    P, Cc, dz, jz, F, G, iz = proto.sides(shape)[0]
    assert dz.size == 0
    for i in (0, 77):
        p, c = tuple(m[i] for m in P), tuple(m[i] for m in Cc)
        assert all(np.array_equal(a, b) for a, b in zip(proto.extend(p, c, dz), cp.stack(p, c)))
        a, b = proto.dconnect(p, c, dz, jz, F[i], G[i], iz), cp.connect(p, c, jz, F[i], G[i], iz)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] == 0


def test_a_delayed_read_breaks_the_algebraic_loop():
    """a one-state plant with D = 1 under F = 1 on its own output: ill-posed now, well-posed one sample late; and the closed form of
    1 / (z - 1) read one sample late under v = -K q + K w"""
    p = (np.array([[0.5]]), np.array([[1.0]]), np.array([[1.0]]), np.array([[1.0]]))
    one = np.array([[1.0]])
    out = proto.dconnect(p, None, [], [0], one, one, None)
    assert out[4] == proto.ILL_POSED and all(np.isnan(m).all() for m in out[:4])
    Phi, Gam, Cm, D, st = proto.dconnect(p, None, [0], [1], one, one, None)
    assert st == 0 and np.array_equal(Phi, [[0.5, 1.0], [1.0, 1.0]]) and np.array_equal(Gam, [[1.0], [1.0]])
    assert np.array_equal(Cm, [[1.0, 1.0], [0.0, 1.0]]) and np.array_equal(D, [[1.0], [0.0]])
    assert proto.dconnect(p, None, [0], [1], np.array([[np.nan]]), one, None)[4] == proto.NOT_FINITE
    integ = (one, one, one, np.zeros((1, 1)))
    for K in (0.25, 0.5, 2.0):
        Phi, Gam, Cm, D, st = proto.dconnect(integ, None, [0], [1], np.array([[-K]]), np.array([[K]]), [0])
        assert st == 0 and np.array_equal(Phi, [[1.0, -K], [1.0, 0.0]]) and np.array_equal(Gam, [[K], [0.0]]) and np.array_equal(Cm, [[1.0, 0.0]])
        assert (np.abs(np.linalg.eigvals(Phi)).max() < 1.0) == (K < 1.0)


# ---- the generator of the GPU tests --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", proto.SHAPES, ids=proto.ident)
def test_float64_stays_within_1e_14_of_longdouble(shape, capsys):
    """on the very systems tests/test_gpu_dconnect.py runs (proto.sides: N_SYS systems per shape, one draw of the generator)"""
    cs, f, l = proto.sides(shape)
    assert (f[4] == 0).all() and (l[4] == 0).all()
    worst = max(float(proto.block_dev(f[k], l[k]).max()) for k in range(4))
    P, Cc, dz, jz, F, G, iz = cs
    nz, nd = shape[4] + shape[5], shape[6]
    cond = 0.0
    for i in range(F.shape[0]):
        De = proto.extend(tuple(m[i] for m in P), None if Cc is None else tuple(m[i] for m in Cc), dz)[3]
        cond = max(cond, float(np.linalg.cond(np.eye(F.shape[1]) - F[i] @ De[jz])))
    with capsys.disabled():
        print(f"\n[dconnect prototype, float64 vs longdouble] {proto.ident(shape)} x {F.shape[0]} systems: {worst:.2e} of the block's largest "
              f"entry; cond(E) <= {cond:.2f}", end="")
    assert len(set(jz.tolist())) == len(jz) and len(set(iz.tolist())) == len(iz) and dz.size == nd
    assert nd == 0 or (jz >= nz).any()
    assert nd == 0 or len(jz) < 2 or (jz < nz).any()
    assert cond <= 3.0 + 1e-9
    assert worst <= 1e-14


@pytest.mark.parametrize("shape", proto.SHAPES, ids=proto.ident)
def test_twelve_ticks_meet_the_tick_by_tick_reference(shape, capsys):
    w, ref, got = proto.tick_sides(shape)
    assert w.shape[1] == 12 and np.isfinite(ref).all() and ref.any()
    dev = float(proto.run_dev(got, ref).max())
    with capsys.disabled():
        print(f"\n[dconnect prototype vs tick-by-tick simulation] {proto.ident(shape)} x {w.shape[0]} systems, 12 ticks: {dev:.2e} of the largest output", end="")
    assert dev <= TICK_BOUND
