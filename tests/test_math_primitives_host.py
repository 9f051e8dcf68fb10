"""The math primitives of csrc/c172_device_impl.inc on the host: their shipped TEXT is cut out of the file (never a copy), compiled with g++
behind the op codes of fb_math_probe, and measured over the sets of tests/math_cases.py against long double references. The hardware
builtins get correctly rounded stand-ins (v_rsq_f64: 1 / sqrtl rounded; v_rcp_f32: 1.0f / x; v_exp_f32, v_log_f32: exp2 / log2 rounded;
the LDS table: atanl rounded; the float-to-int conversion: the hardware's, NaN -> 0 and saturating), so what is measured is H, the error of
the ARITHMETIC as written — what the device adds to it is its seeds and its <= 1-ulp division, which tests/test_gpu_math_primitives.py
measures against bounds fixed from the H recorded in math_cases.py. Measured with floating-point contraction off and on (the device
contracts). This file took over the sincos_step test of test_math_kernels.py, asserts unchanged."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import math_cases as mc
from oracle_binding import header_enums
from support import ROOT

CSRC = os.path.join(ROOT, "flight.jl_amd", "csrc")
SRC = os.path.join(CSRC, "c172_device_impl.inc")
K = header_enums()
LD = np.longdouble

PRELUDE = r"""
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <type_traits>
#define FBD inline
#define FBL(x) ((real)(x))
#define FB_ST_ISA_RANGE %d
static double g_seed_rel = 0.0;   // the rsq seed's relative error, for the sensitivity runs: this value, or (g_seed_rand) uniform within +- it
static int g_seed_rand = 0;
static unsigned long long g_lcg = 1;
static inline double host_rsq(double x) {
    long double e = g_seed_rel;
    if (g_seed_rand) { g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL; e *= (double)(g_lcg >> 11) * 0x1p-52 - 1.0; }
    return (double)((1.0L / sqrtl((long double)x)) * (1.0L + e));
}
static inline float host_rcpf(float x) { return 1.0f / x; }
static inline float host_rintf(float x) { return x != x ? 0.0f : fminf(fmaxf(rintf(x), -2147483520.0f), 2147483520.0f); }   // then (int) as v_cvt_i32_f32
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
#define __builtin_amdgcn_rsq(x) host_rsq(x)
#define __builtin_amdgcn_rcpf(x) host_rcpf(x)
#define __builtin_rintf(x) host_rintf(x)
#define __builtin_amdgcn_exp2f(x) ((float)exp2((double)(x)))
#define __builtin_amdgcn_logf(x) ((float)log2((double)(x)))
"""
INSTANCE = r"""
namespace %s {
typedef %s real;
typedef const real* lds_cptr;
constexpr int ATAN_N = 33;   // (its definition sits among the LDS layout constants, outside the stretches cut out; shipped_text() checks the value)
%s
}
"""
ENTRY = r"""
extern "C" void mp_seed(double rel, int rnd, unsigned long long start) { g_seed_rel = rel; g_seed_rand = rnd; g_lcg = start; }
extern "C" int mp_eval(int op, long n, const double* pa, const double* pb, double* o0, double* o1) {
    double tab[33];
    for (int k = 0; k < 33; k++) tab[k] = (double)atanl(k / 32.0L);
    for (long i = 0; i < n; i++) {
        const double a = pa[i], b = pb ? pb[i] : 0.0;
        const float af = (float)a, bf = (float)b;
        double r0 = 0.0, r1 = 0.0;
        switch (op) {
        case FB_MP_SQRT: r0 = fbd::sqrt(a); break;
        case FB_MP_RSQRT: r0 = fbd::rsqrt(a); break;
        case FB_MP_HALF_ANGLE: fbd::half_angle_cs(a, b, r0, r1); break;
        case FB_MP_ATAN2_TAB: r0 = fbd::atan2_step(a, b, tab); break;
        case FB_MP_ATAN2_TAB_XPOS: r0 = fbd::atan2_step<true>(a, b, tab); break;
        case FB_MP_LOG_NEAR1: r0 = fbd::log_near1(a); break;
        case FB_MP_SINCOS_STEP: fbd::sincos_step(a, r0, r1); break;
        case FB_MP_ISA_FAST:
        case FB_MP_ISA: {
            double T, pr, lnp;
            int32_t st = 0;
            if (op == FB_MP_ISA_FAST) fbd::isa_data<true>(a, b, 1.0, T, pr, lnp, st); else fbd::isa_data<false>(a, b, 1.0, T, pr, lnp, st);
            o0[i] = T; o0[n + i] = pr; o0[2 * n + i] = lnp; o1[i] = (double)st;
            continue;
        }
        case FB_MP_DIV: r0 = a / b; break;   // (the host's own, correctly rounded: for the special values only)
        case FB_MP_F32_ATAN2_FAST: r0 = fbf::atan2_step(af, bf, nullptr); break;
        case FB_MP_F32_ATAN2_FAST_XPOS: r0 = fbf::atan2_step<true>(af, bf, nullptr); break;
        case FB_MP_F32_EXP_STEP: r0 = fbf::exp_step(af); break;
        case FB_MP_F32_LOG_STEP: r0 = fbf::log_step(af); break;
        default: return -1;
        }
        o0[i] = r0;
        if (o1) o1[i] = r1;
    }
    return 0;
}
"""


def shipped_text():
    """the three stretches of c172_device_impl.inc that hold the primitives: constants, sqrt, rsqrt | half_angle_cs .. sincos_step | the ISA"""
    text = open(SRC, encoding="utf-8").read()
    cuts = []
    for a, b in ((r"^constexpr real PI = ", r"^// -+\n// small vector"), (r"^// cos and sin of atan2\(y, x\) / 2 without", r"^FBD void sincos_step\(float"),
                 (r"^namespace isa \{", r"^// -+\n// continuous PI compensator")):
        m, e = re.search(a, text, flags=re.M), re.search(b, text, flags=re.M)
        assert m and e and m.start() < e.start(), (a, b)
        cuts.append(text[m.start():e.start()])
    body = "\n".join(cuts)
    assert "constexpr int LDS_ATAN = LDS_RK_KNOTS, ATAN_N = 33;" in text
    for name in ("FBD real sqrt(", "FBD real rsqrt(", "FBD void half_angle_cs(", "FBD double atan2_tab(", "FBD float atan2_fast(", "FBD double log_near1(",
                 "FBD void sincos_step(double", "FBD void isa_data(", "FBD real exp_step(", "FBD real log_step("):
        assert body.count(name) == 1, name
    return body


class HostLib:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.mp_seed.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_ulonglong]

    def run(self, op, a, b=None):
        P = ctypes.POINTER(ctypes.c_double)
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        isa = op in mc.ISA_OPS
        o0, o1 = np.empty((3, a.size) if isa else a.size), np.empty(a.size)
        rc = self.lib.mp_eval(K[op], ctypes.c_long(a.size), a.ctypes.data_as(P), None if b is None else b.ctypes.data_as(P), o0.ctypes.data_as(P), o1.ctypes.data_as(P))
        assert rc == 0, op
        return o0, o1

    def seed(self, rel, draw=None):
        """the rsq stand-in's relative error: `rel` for every call, or (draw: a number) uniform within +-rel, a new value per call"""
        self.lib.mp_seed(rel, 0 if draw is None else 1, 0 if draw is None else 2 * draw + 1)


def has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """contraction -> HostLib: "off" always; "on" where the CPU has fused multiply-add (without it g++ has nothing to contract into)"""
    d = tmp_path_factory.mktemp("mp")
    body = shipped_text()
    defs = "".join("#define %s %d\n" % (k, v) for k, v in K.items() if k.startswith("FB_MP_"))
    src = d / "h.cpp"
    src.write_text(PRELUDE % K["FB_ST_ISA_RANGE"] + defs + INSTANCE % ("fbd", "double", body) + INSTANCE % ("fbf", "float", body) + ENTRY)
    libs = {}
    for name, flags in (("off", ["-ffp-contract=off"]), ("on", ["-ffp-contract=fast", "-mfma"])):
        if name == "on" and not has_fma():
            print("\n(no fused multiply-add on this CPU: contraction-on figures not measured here)")
            continue
        so = d / f"h_{name}.so"
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", *flags, "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
        libs[name] = HostLib(str(so))
    return libs


def test_preconditions_long_double_and_references():
    """before anything else: long double is the x87 format, and its library functions are a reference (within 2^-8 ulp of 50 digits)"""
    assert np.finfo(LD).nmant == 63 and np.finfo(LD).eps == LD(2) ** -63
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    f = {"FB_MP_SQRT": lambda a: (mp.sqrt(a),), "FB_MP_RSQRT": lambda a: (1 / mp.sqrt(a),), "FB_MP_DIV": lambda a, b: (a / b,), "FB_MP_RCP": lambda a: (1 / a,),
         # (the principal square root of the unit complex number: cos and sin of half its argument, each to full relative accuracy)
         "FB_MP_HALF_ANGLE": lambda y, x: (lambda z: (z.real, z.imag))(mp.sqrt(mp.mpc(x, y) / mp.hypot(x, y))),
         "FB_MP_LOG_NEAR1": lambda a: (mp.log(a),), "FB_MP_SINCOS_STEP": lambda a: (mp.sin(a), mp.cos(a)),
         "FB_MP_LIB_EXP": lambda a: (mp.exp(a),), "FB_MP_LIB_LOG": lambda a: (mp.log(a),), "FB_MP_F32_EXP_STEP": lambda a: (mp.exp(a),), "FB_MP_F32_LOG_STEP": lambda a: (mp.log(a),),
         "FB_MP_F32_SQRT": lambda a: (mp.sqrt(a),), "FB_MP_F32_RSQRT": lambda a: (1 / mp.sqrt(a),), "FB_MP_F32_DIV": lambda a, b: (a / b,)}
    at = lambda y, x: (mp.atan2(y, x),)
    for op in ("FB_MP_ATAN2_TAB", "FB_MP_ATAN2_TAB_XPOS", "FB_MP_LIB_ATAN2", "FB_MP_F32_ATAN2_FAST", "FB_MP_F32_ATAN2_FAST_XPOS"):
        f[op] = at
    f["FB_MP_LIB_SINCOS"] = f["FB_MP_SINCOS_STEP"]
    assert set(f) == set(mc.CASES)

    def as_mp(v):                           # a long double, exactly: its mantissa split into two doubles
        m, e = np.frexp(v)
        hi = np.float64(m)
        return (mp.mpf(float(hi)) + mp.mpf(float(np.float64(m - LD(hi))))) * mp.mpf(2) ** int(e)

    def rel_ulps(ref_ld, exact, mant):      # |ref - exact| in ulps of the op's format, the difference taken at 50 digits
        r = as_mp(ref_ld)
        if exact == 0:
            return 0.0 if r == 0 else np.inf
        return float(abs(r - exact) / mp.mpf(2) ** (int(mp.floor(mp.log(abs(exact), 2))) - mant))
    for op, c in mc.CASES.items():
        ins, ref = c.inputs(), c.ref()
        idx = np.random.default_rng(1).choice(ins[0].size, 2000, replace=False)
        worst = 0.0
        for i in idx:
            exact = f[op](*(mp.mpf(float(a[i])) for a in ins))
            worst = max(worst, max(rel_ulps(r[i], x, c.mant) for r, x in zip(ref, exact)))
        assert worst <= 2.0 ** -8, (op, worst)
    # the ISA reference and the table the same way
    h, T = mc.isa_inputs()
    ref = mc.isa_ref()
    R, g = mp.mpf(mc.ISA_R), mp.mpf(mc.ISA_G)
    worst = 0.0
    for i in np.random.default_rng(2).choice(h.size, 2000, replace=False):
        if h[i] >= mc.ISA_HC[-1]:
            continue
        hb, Tb, lnp, hi = mp.mpf(0), mp.mpf(float(T[i])), mp.mpf(0), mp.mpf(float(h[i]))
        for beta, hc in zip(mc.ISA_BETA, mc.ISA_HC):
            beta, hh = mp.mpf(float(beta)), min(hi, mp.mpf(float(hc)))
            lnp += -g / (beta * R) * mp.log(1 + beta / Tb * (hh - hb)) if beta != 0 else -g / (R * Tb) * (hh - hb)
            Tn = Tb + beta * (hh - hb)
            if hi < hc:
                break
            hb, Tb = mp.mpf(float(hc)), Tn
        # in the units of the bounds (2^-44 K, 2^-52 relative, 2^-52): the long double sum lnp reaches -16, where its own rounding is 2^-60,
        # and p = exp(lnp) inherits that as a relative error — 2^-8 of a unit per term, against bounds of 18 units and more
        worst = max(worst, float(abs(as_mp(ref[0][i]) - Tn)) * 2.0 ** 44, float(abs(as_mp(ref[1][i]) / mp.exp(lnp) - 1)) * 2.0 ** 52,
                    float(abs(as_mp(ref[2][i]) - lnp)) * 2.0 ** 52)
    assert worst <= 2.0 ** -4, ("isa", worst)
    for k in range(33):
        assert rel_ulps(mc.table_ref()[k], mp.atan(mp.mpf(k) / 32), 52) <= 2.0 ** -8


def test_caller_range_of_log_near1_is_inside_its_domain():
    """u0 = 1 + beta0 / T_sl h0: h0 is capped at 11 km, T_sl saturates (sat_T_sl), a lane below H_MIN is flagged"""
    capi = open(os.path.join(CSRC, "fb_capi.hip"), encoding="utf-8").read()
    impl = open(SRC, encoding="utf-8").read()
    assert "static double sat_T_sl(double T) { return fmin(fmax(T, isa::T_std - 50.0), isa::T_std + 50.0); }" in capi
    assert "constexpr real H_MIN = -FBL(1000.0);" in impl and "const real h0 = fmin(h, kc<KC_ISA_H11>(K));" in impl
    assert mc.T_SL_RANGE == (288.15 - 50.0, 288.15 + 50.0)
    h_gp_min = -1000.0 * 6378137.0 / (6378137.0 - 1000.0)     # the geopotential altitude of H_MIN
    lo, hi = 1 - 6.5e-3 * 11000.0 / mc.T_SL_RANGE[0], 1 - 6.5e-3 * h_gp_min / mc.T_SL_RANGE[0]
    assert mc.LOG_NEAR1_CALLER[0] <= lo and hi <= mc.LOG_NEAR1_CALLER[1], (lo, hi)
    assert mc.LOG_NEAR1_DOMAIN[0] <= mc.LOG_NEAR1_CALLER[0] and mc.LOG_NEAR1_CALLER[1] <= mc.LOG_NEAR1_DOMAIN[1]


def test_atan2_fast_polynomial_error_is_what_its_bound_counts():
    """t P(t^2) against atan t on [0, 1] in long double, with the coefficients as the source has them: the first term of ATAN2_FAST_BOUND"""
    text = open(SRC, encoding="utf-8").read()
    for c in mc.ATAN2_FAST_COEF:
        assert "%sf" % repr(c) in text, c
    t = np.linspace(LD(0), LD(1), 1_000_001)
    p = LD(0)
    for c in mc.ATAN2_FAST_COEF:
        p = p * (t * t) + LD(float(np.float32(c)))
    e = float(np.abs(t * p - np.arctan(t)).max())
    print("\natan2_fast: polynomial error %.3e (counted as %.2e)" % (e, mc.ATAN2_FAST_POLY), end="")
    assert e <= mc.ATAN2_FAST_POLY and mc.ATAN2_FAST_POLY - e <= 2e-9


def test_isa_exp_series_truncation():
    """isa_data<true>'s degree-9 exp series on |y| <= 0.1 (y = 0.256 ln u0, |ln u0| <= 0.357): the coefficients are 1/k! in the source, and
    what the series leaves out is 2.8e-17, the figure its comment gives"""
    text = open(SRC, encoding="utf-8").read()
    fact = {3: 6, 4: 24, 5: 120, 6: 720, 7: 5040, 8: 40320, 9: 362880}
    for k, f in fact.items():
        assert "FB_KC(KC_EXP_C%d, FBL(1.0) / %d)" % (k, f) in text, k
    assert 0.256 * 0.357 < 0.1
    y = np.linspace(LD(-0.1), LD(0.1), 200_001)
    e = LD(1) / 362880
    for k in (8, 7, 6, 5, 4, 3):
        e = e * y + LD(1) / fact[k]
    e = ((e * y + LD(0.5)) * y + 1) * y + 1
    t = float(np.abs(e - np.exp(y)).max())
    print("\nisa_data<true>: exp series truncation %.2e" % t, end="")
    assert 2.7e-17 <= t <= 2.9e-17      # (0.1^10 / 10! (1 + 0.1 / 11) = 2.78e-17; the long double's own rounding, a few 1e-19, on top)


def test_sincos_step_accuracy(host):
    """(from test_math_kernels.py, asserts as they were: <= 1.5 ulp on each of the five sets, NaN and the infinities give NaN)"""
    for name, x in mc.sincos_sets():
        s, c = host["off"].run("FB_MP_SINCOS_STEP", x)
        es, ec = mc.ulps(s, np.sin(LD(1) * x)), mc.ulps(c, np.cos(LD(1) * x))
        print("%-58s max error: sin %.2f ulp, cos %.2f ulp" % (name, es.max(), ec.max()))
        assert es.max() <= 1.5 and ec.max() <= 1.5, (name, es.max(), ec.max())
    s, c = host["off"].run("FB_MP_SINCOS_STEP", np.array([np.nan, np.inf, -np.inf]))
    assert np.isnan(s).all() and np.isnan(c).all()


def worst_of(case, outs):
    errs = case.errors(outs)
    w = [(float(e.max()), int(e.argmax())) for e in errs]
    k = int(np.argmax([x[0] for x in w]))
    ins = case.inputs()
    return w[k][0], tuple(float(a[w[k][1]]) for a in ins)


@pytest.mark.parametrize("op", mc.HOST_OPS)
def test_host_worst_case_is_what_math_cases_records(host, op):
    """H per op, contraction off and on, printed with its argument; the record in math_cases.py (which fixes the device bounds) covers it"""
    case = mc.CASES[op]
    H = {}
    for mode, lib in host.items():
        o0, o1 = lib.run(op, *case.inputs())
        H[mode], arg = worst_of(case, (o0, o1))
        assert case.regions is None or case.within(case.errors((o0, o1))), (op, mode, "a region's own bound")
        print("\n%-28s contraction %-3s H = %.4g %s at %s" % (op, mode, H[mode], case.measure, " ".join(x.hex() for x in arg)), end="")
    recorded = case.H if case.H is not None else case.fixed
    assert max(H.values()) <= recorded, (op, H, recorded)
    if case.H is not None and op not in mc.SEEDED_OPS:
        assert case.H - max(H.values()) <= 0.02 or "on" not in H, ("the record is stale: it fixes the device's bound", op, H, case.H)


@pytest.mark.parametrize("op", mc.SEEDED_OPS)
def test_seed_sensitivity(host, op):
    """The rsq seed moved by +-2^-28, +-2^-26, +-2^-24 and +-2^-23 relative, and by a fresh error uniform within +-2^-23 at every call (twelve
    draws): the spread is printed. sqrt does not move at all. rsqrt and half_angle_cs DO: the correctly rounded seed is a special case (the
    Newton steps then have next to nothing to correct), any other seed costs rsqrt a quarter of an ulp (it stays below its claim of 1) and
    half_angle_cs, two rsqrt deep, up to half an ulp. So for these ops the H that math_cases.py records is the worst over all these runs:
    the device's seed is one of them, not the correctly rounded one."""
    case = mc.CASES[op]
    lib = host.get("on", host["off"])
    spread = {}
    try:
        for p in (0, -28, -26, -24, -23):
            for sgn in ((0,) if p == 0 else (-1, 1)):
                lib.seed(sgn * 2.0 ** p)
                spread["exact" if p == 0 else "%s2^%d" % ("+" if sgn > 0 else "-", p)] = worst_of(case, lib.run(op, *case.inputs()))[0]
        for draw in range(12):
            lib.seed(2.0 ** -23, draw)
            spread["uniform 2^-23 #%d" % draw] = worst_of(case, lib.run(op, *case.inputs()))[0]
    finally:
        lib.seed(0.0)
    print("\n%-18s worst ulp by relative seed error: %s" % (op, "  ".join("%s %.4f" % kv for kv in spread.items())), end="")
    assert max(spread.values()) <= case.H and (case.H - max(spread.values()) <= 0.02 or "on" not in host), (spread, case.H)
    if op == "FB_MP_SQRT":
        assert max(spread.values()) - spread["exact"] <= 0.01, spread


@pytest.mark.parametrize("op", mc.ISA_OPS)
def test_isa_data_within_its_bounds(host, op):
    h, T = mc.isa_inputs()
    for mode, lib in host.items():
        o0, st = lib.run(op, h, T)
        errs, bounds, ok = mc.isa_errors(o0, mc.isa_ref(), h)
        for name, e, b in zip(("T [2^-44]", "p rel [2^-52]", "lnp [2^-52]"), errs, bounds):
            k = int(np.argmax(e / b))
            print("\n%-14s contraction %-3s %-14s worst %.2f of bound %.0f at h = %r, T_sl = %r" % (op, mode, name, e[k], b[k], h[ok][k], T[ok][k]), end="")
            assert (e <= b).all(), (op, mode, name, e[k], b[k])
        assert np.array_equal(st != 0, h >= mc.ISA_HC[-1]) and set(np.unique(st)) <= {0.0, float(K["FB_ST_ISA_RANGE"])}


def test_special_values(host):
    for lib in host.values():
        bad = mc.check_specials(lambda op, a, b: lib.run(op, a, b), ops=set(mc.HOST_OPS) | {"FB_MP_DIV"})
        assert not bad, "\n".join(map(str, bad))


def test_probe_refusals(fb):
    """decided on the host before anything touches a device"""
    P = ctypes.POINTER(ctypes.c_double)
    a = np.ones(4); o = np.zeros(12)
    pa, po = a.ctypes.data_as(P), o.ctypes.data_as(P)
    err = lambda: fb.lib.fb_last_error()
    for op in (-1, K["FB_MP_F64_END"], K["FB_MP_F64_END"] + 3, K["FB_MP_F32_END"], 1000):
        assert fb.lib.fb_math_probe(op, 4, pa, pa, po, po) != 0 and b"fb_math_probe: unknown op" in err(), (op, err())
    assert fb.lib.fb_math_probe(K["FB_MP_SQRT"], 0, pa, None, po, None) != 0 and b"1 <= n" in err()
    assert fb.lib.fb_math_probe(K["FB_MP_SQRT"], K["FB_MP_N_MAX"] + 1, pa, None, po, None) != 0 and b"1 <= n" in err()
    assert fb.lib.fb_math_probe(K["FB_MP_SQRT"], 4, None, None, po, None) != 0 and b"null a or out0" in err()
    assert fb.lib.fb_math_probe(K["FB_MP_SQRT"], 4, pa, None, None, None) != 0 and b"null a or out0" in err()
    for op in ("FB_MP_DIV", "FB_MP_ATAN2_TAB", "FB_MP_ISA", "FB_MP_F32_DIV"):
        assert fb.lib.fb_math_probe(K[op], 4, pa, None, po, po) != 0 and b"b is null" in err(), op
    for op in ("FB_MP_HALF_ANGLE", "FB_MP_SINCOS_STEP", "FB_MP_LIB_SINCOS", "FB_MP_ISA_FAST"):
        assert fb.lib.fb_math_probe(K[op], 4, pa, pa, po, None) != 0 and b"out1 is null" in err(), op
    assert set(k for k in K if k.startswith("FB_MP_") and not k.endswith(("_END", "_N_MAX"))) == set(mc.CASES) | set(mc.ISA_OPS) | {"FB_MP_ATAN_TABLE"}
