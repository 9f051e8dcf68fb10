"""The device math primitives of csrc/c172_device_impl.inc ON THE DEVICE, through fb_math_probe (csrc/fb_mathprobe.inc: one kernel in the
shipped library, so the primitives are compiled with the shipped flags): each op over the ~10^6 seeded inputs of tests/math_cases.py against
the same long double reference the host test uses, the worst error printed with its argument and held to the bound that math_cases.py fixed
beforehand (B = max(claim, H + 0.5 ulp per fp64 division); division 1 ulp; fp32 the source's claims) — never one read off the device.
Also: a ragged batch gives the bits of the full one, the staged atan table against atanl, the special-value table, and isa_data's two forms
against the long double ISA, against each other and with FB_ST_ISA_RANGE exactly from 84 852 m."""
import ctypes as C

import numpy as np
import pytest

import math_cases as mc

pytestmark = pytest.mark.gpu
_D = C.POINTER(C.c_double)
LD = np.longdouble


def probe(fb, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    o0, o1 = np.full((3, a.size) if op in mc.ISA_OPS else a.size, np.nan), np.full(a.size, np.nan)
    rc = fb.lib.fb_math_probe(fb.K[op], a.size, a.ctypes.data_as(_D), None if b is None else b.ctypes.data_as(_D), o0.ctypes.data_as(_D), o1.ctypes.data_as(_D))
    assert rc == 0, (op, fb.lib.fb_last_error())
    return o0, o1


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def assert_ragged(fb, op, ins, full):
    """the first 1, 63 and 65 inputs alone: the bits they have inside the full batch"""
    for m in (1, 63, 65):
        part = probe(fb, op, *(x[:m] for x in ins))
        for p, f in zip(part, full):
            assert same_bits(p[..., :m], f[..., :m]), (op, m)


@pytest.mark.parametrize("op", list(mc.CASES))
def test_accuracy(fb, op):
    case = mc.CASES[op]
    ins = case.inputs()
    assert ins[0].size % 64 != 0            # a ragged last wave
    outs = probe(fb, op, *ins)
    errs = case.errors(outs)
    worst = max(((float(e.max()), int(e.argmax()), k) for k, e in enumerate(errs)))
    arg = " ".join(float(x[worst[1]]).hex() for x in ins)
    print("\n%-28s device worst %.4g %s (output %d) at %s; bound %.4g; domain %s" % (op, worst[0], case.measure, worst[2], arg, case.bound, case.domain), end="")
    assert worst[0] <= case.bound, (op, worst[0], case.bound, arg)
    assert case.within(errs), (op, "a region's own bound")
    assert_ragged(fb, op, ins, outs)


def test_atan_table(fb):
    """the 33 staged entries within 1 ulp of atanl(k / 32), entry by entry; an index outside 0 .. 32 is clamped"""
    k = np.arange(-2, 36, dtype=np.float64)
    got, _ = probe(fb, "FB_MP_ATAN_TABLE", k)
    ref = mc.table_ref()
    e = mc.ulps(got[2:35], ref)
    print("\natan table: worst %.3f ulp at k = %d" % (e.max(), int(e.argmax())), end="")
    assert (e <= 1.0).all() and got[2] == 0.0, e
    assert got[0] == got[1] == got[2] and got[35] == got[36] == got[37] == got[34]


def test_special_values(fb):
    bad = mc.check_specials(lambda op, a, b: probe(fb, op, a, b))
    assert not bad, "\n".join(map(str, bad))
    for op in mc.ISA_OPS:       # a NaN altitude is below no layer's ceiling: flagged
        _, st = probe(fb, op, np.array([np.nan]), np.array([288.15]))
        assert int(st[0]) == fb.K["FB_ST_ISA_RANGE"]


_ISA = {}


def isa_run(fb, op):
    if op not in _ISA:
        _ISA[op] = probe(fb, op, *mc.isa_inputs())
    return _ISA[op]


@pytest.mark.parametrize("op", mc.ISA_OPS)
def test_isa_data(fb, op):
    h, T_sl = mc.isa_inputs()
    o0, st = isa_run(fb, op)
    errs, bounds, ok = mc.isa_errors(o0, mc.isa_ref(), h)
    for name, e, b in zip(("T [2^-44]", "p rel [2^-52]", "lnp [2^-52]"), errs, bounds):
        k, w = int(np.argmax(e / b)), int(np.argmax(e))
        print("\n%-14s %-14s device worst %.2f at h = %r, T_sl = %r; nearest its bound: %.2f of %.0f at h = %r, T_sl = %r"
              % (op, name, e[w], h[ok][w], T_sl[ok][w], e[k], b[k], h[ok][k], T_sl[ok][k]), end="")
        assert (e <= b).all(), (op, name, e[k], b[k], h[ok][k], T_sl[ok][k])
    # FB_ST_ISA_RANGE exactly from 84 852 m (the reference throws for h >= the last ceiling), and no other bit
    assert np.array_equal(st != 0, h >= mc.ISA_HC[-1]) and set(np.unique(st)) <= {0.0, float(fb.K["FB_ST_ISA_RANGE"])}
    assert (h >= mc.ISA_HC[-1]).sum() >= 80 and (h == np.nextafter(mc.ISA_HC[-1], 0)).sum() >= 40
    assert_ragged(fb, op, (h, T_sl), (o0, st))


def test_isa_data_fast_against_plain(fb):
    """the two forms against each other: within the sum of their bounds, and the same flags"""
    h, _ = mc.isa_inputs()
    (f0, fst), (p0, pst) = isa_run(fb, "FB_MP_ISA_FAST"), isa_run(fb, "FB_MP_ISA")
    errs, bounds, ok = mc.isa_errors(f0, tuple(np.asarray(x, dtype=LD) for x in p0), h)
    for name, e, b in zip(("T", "p", "lnp"), errs, bounds):
        print("\nisa_data<true> - isa_data<false>  %-4s worst %.2f (in the units of its bound)" % (name, e.max()), end="")
        assert (e <= 2 * b).all(), name
    assert np.array_equal(fst, pst)
