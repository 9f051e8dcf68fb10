"""The device math primitives of csrc/c172_device_impl.inc, as cases: per op its seeded inputs, its STATED DOMAIN, a long double reference of
the same operation, the error measure and the bound with its derivation. Shared by tests/test_math_primitives_host.py (the shipped text
compiled for the host, hardware seeds replaced by correctly rounded stand-ins: it measures H) and tests/test_gpu_math_primitives.py (the
device through fb_math_probe). No device work and nothing compiled at import; inputs and references are computed once and never modified.

THE RULE FOR A BOUND (fixed before any device run, never read off the device):
  fp64 ulp ops    B = max(claim, H + 0.5 * ndiv): `claim` is the source comment's figure, H the host worst case recorded below (the larger
                  of contraction off and on, rounded up to 0.01), ndiv the fp64 divisions on the path: the device's quotient is <= 1 ulp
                  where the host's is 0.5. The ops built on v_rsq_f64 (SEEDED_OPS): H is the worst over the host's seed runs, the seed
                  moved by up to 2^-23 relative (sqrt does not move; rsqrt and half_angle_cs do: the device's seed is not the correctly rounded one).
  division        the claim, 1 ulp.
  fp32            the source's claim (divide, sqrt 2.5 ulp; atan2_fast: the claim as corrected below, ATAN2_FAST_BOUND — the "2e-7 absolute" it
                  replaces is already missed on the host); exp_step / log_step: an absolute bound derived below.
  library exp, log, sincos, atan2 (fp64, as the hot path compiles them): the OpenCL full-profile limits the device library documents
                  that it meets (3, 3, 4, 6 ulp); the project states no claim of its own and the host cannot compile that library.
  isa_data        absolute / relative bounds per layer from a rounding-error count (ISA_LNP_BOUND below).
ulp(ref) = 2^(ilogb|ref| - 52) (fp32: - 23), as in the sincos_step test this file's sets came from."""
import numpy as np

LD = np.longdouble
N = 2 ** 20 + 37                      # a ragged last wave
PI_D, HALF_PI_D = 3.141592653589793, 1.5707963267948966
PI_F, HALF_PI_F = float(np.float32(3.141592653589793)), float(np.float32(1.5707963267948966))
ISA_HC = np.array([11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0, 84852.0])
ISA_BETA = np.array([-6.5e-3, 0.0, 1e-3, 2.8e-3, 0.0, -2.8e-3, -2e-3])
ISA_R, ISA_G = 287.05287, 9.80665
T_SL_RANGE = (288.15 - 50.0, 288.15 + 50.0)   # fb_set_params / fb_set_env saturate T_sl to 288.15 +- 50 K (sat_T_sl, csrc/fb_capi.hip)
H_RANGE = (-1000.0, 84852.0)          # below H_MIN a lane is flagged FB_ST_ALT_RANGE, at and above 84 852 m FB_ST_ISA_RANGE
FB_ST_ISA_RANGE = 2

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


# ---- error measures ---------------------------------------------------------------------------------------------------------------------
def ulps(got, ref, mant=52):
    """|got - ref| / 2^(ilogb|ref| - mant), in long double; ref = 0 wants got = 0; a non-finite got is an infinite error"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    e = np.frexp(np.abs(ref))[1].astype(np.int64) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - ref) / np.ldexp(LD(1), e - mant)
    err = np.where(ref == 0, np.where(got == 0, LD(0), LD(np.inf)), err)
    return np.where(np.isfinite(got), err, LD(np.inf)).astype(np.float64)


def abs_err(got, ref):
    got = np.asarray(got, dtype=LD)
    return np.where(np.isfinite(got), np.abs(got - np.asarray(ref, dtype=LD)), LD(np.inf)).astype(np.float64)


# ---- input sets -------------------------------------------------------------------------------------------------------------------------
def _logu(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def _sign(rng, n):
    return rng.choice(np.array([-1.0, 1.0]), n)


def _move(x, k):
    """x moved by k units in the last place, away from zero for k > 0 (float64 or float32 arrays of non-zero finite numbers)"""
    it = np.int64 if x.dtype == np.float64 else np.int32
    return (np.ascontiguousarray(x).view(it) + np.asarray(k).astype(it)).view(x.dtype)


def _fill(parts, n, more):
    """concatenate the parts and bring them to n elements with more(m)"""
    have = sum(p[0].size for p in parts)
    assert have <= n, (have, n)
    if have < n:
        parts.append(more(n - have))
    return tuple(np.ascontiguousarray(np.concatenate([p[j] for p in parts])) for j in range(len(parts[0])))


ATAN2_DOMAIN = (1e-30, 1e30)   # of max(|x|, |y|): the quotient's single-precision estimate needs it inside fp32's normal range (or x = y = 0)


def _atan2_inputs(seed, f32=False, xpos=False):
    rng = np.random.default_rng(seed)
    lo, hi = ATAN2_DOMAIN
    rel = 1e-6 if f32 else 1e-9

    def polar(m, rlo, rhi):
        th, r = rng.uniform(-np.pi, np.pi, m), _logu(rng, rlo, rhi, m)
        return r * np.sin(th), r * np.cos(th)
    parts = [polar(300_000, 2 * lo, hi / 2)]                                               # every angle at every magnitude
    parts.append((_logu(rng, lo, hi, 150_000) * _sign(rng, 150_000), _logu(rng, lo, hi, 150_000) * _sign(rng, 150_000)))   # independent magnitudes
    x = _logu(rng, lo, hi / 2, 50_000) * _sign(rng, 50_000)
    parts.append((x * (1 + rel * rng.uniform(-1, 1, 50_000)) * _sign(rng, 50_000), x))         # y = +-x (1 +- rel): the octant boundary
    # quotients at and next to every k / 32 and (k + 1/2) / 32, k = 0 .. 32: the table's knots and the points where the estimate changes entry
    g = np.repeat(np.concatenate([np.arange(33) / 32.0, (np.arange(33) + 0.5) / 32.0]), 1500)
    d = np.where(rng.random(g.size) < 0.5, rng.integers(-3, 4, g.size) * 2.0 ** -52, rng.uniform(-1, 1, g.size) * 2.0 ** -20)
    mx = _logu(rng, 4 * lo, hi / 4, g.size)
    mn = g * (1 + d) * mx
    sw = rng.random(g.size) < 0.5
    parts.append((np.where(sw, mx, mn) * _sign(rng, g.size), np.where(sw, mn, mx) * _sign(rng, g.size)))
    big = _logu(rng, 1e-14, hi, 150_000)
    parts.append((big * 10.0 ** -rng.uniform(0, 15, 150_000) * _sign(rng, 150_000), big * _sign(rng, 150_000)))   # |y| << |x|: near 0 and near +-pi
    big = _logu(rng, 1e-14, hi, 100_000)
    parts.append((big * _sign(rng, 100_000), big * 10.0 ** -rng.uniform(0, 15, 100_000) * _sign(rng, 100_000)))   # |x| << |y|: near +-pi/2
    y, x = _fill(parts, N, lambda m: polar(m, 0.1, 10.0))
    if f32:
        y, x = y.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64)
    if xpos:
        x = np.abs(x)
    mxa = np.maximum(np.abs(x), np.abs(y))
    assert mxa.min() >= lo and mxa.max() <= hi
    return y, x


def _sqrt_inputs(seed, f32=False):
    rng = np.random.default_rng(seed)
    lo, hi, kmax, e0, e1 = (1e-37, 1e38, 2 ** 12, -122, 127) if f32 else (1e-280, 1e300, 2 ** 26, -929, 997)
    ft = np.float32 if f32 else np.float64
    sq = rng.integers(1, kmax, 100_000).astype(ft) ** 2                                       # perfect squares (exact) and their neighbours
    p2 = (2.0 ** np.arange(e0, e1)).astype(ft)                                                # powers of two and one ulp either side
    parts = [(_logu(rng, lo, hi, 700_000).astype(ft),), (sq,), (_move(sq, -1),), (_move(sq, 1),), (p2,), (_move(p2, -1),), (_move(p2, 1),)]
    (x,) = _fill(parts, N, lambda m: (rng.uniform(1.0, 4.0, m).astype(ft),))
    x = x.astype(np.float64)
    assert x.min() >= lo * 0.99 and x.max() <= hi
    return (x,)


def _div_inputs(seed, f32=False):
    rng = np.random.default_rng(seed)
    emax, mant, ft = (60, 23, np.float32) if f32 else (300, 52, np.float64)

    def rnd(m):
        return (rng.uniform(1.0, 2.0, m) * 2.0 ** rng.integers(-emax, emax + 1, m) * _sign(rng, m)).astype(ft)
    p2 = (2.0 ** rng.integers(-emax, emax + 1, 200_000) * _sign(rng, 200_000)).astype(ft)
    near = _move(p2, np.where(p2 != 0, rng.integers(-1, 2, 200_000), 0))                      # divisors at and one ulp either side of powers of two
    a = rnd(248_000)
    k = np.where(rng.random(248_000) < 0.5, rng.integers(-1000, 1001, 248_000) * 2.0 ** -mant, rng.uniform(-1, 1, 248_000) * (1e-5 if f32 else 1e-9))
    parts = [(rnd(600_000), rnd(600_000)), (rnd(200_000), near), (a, (a.astype(np.float64) * (1 + k)).astype(ft))]   # ..., quotients near 1
    a, b = _fill(parts, N, lambda m: (rnd(m), rnd(m)))
    return a.astype(np.float64), b.astype(np.float64)


LOG_NEAR1_DOMAIN = (0.65, 1.5)      # where the ten-term series holds its accuracy (12 ulp off at 0.6 already)
LOG_NEAR1_CALLER = (0.6997, 1.03)   # u0 = 1 - 6.5e-3 h0 / T_sl over h0 in [-1000.2, 11000] m, T_sl in [238.15, 338.15] K: 0.69977 .. 1.0273


def _log_near1_inputs(seed):
    rng = np.random.default_rng(seed)
    k = np.arange(1, 17)
    edge = np.concatenate([1 - 10.0 ** -k, 1 + 10.0 ** -k, [1.0]])
    return (np.concatenate([rng.uniform(*LOG_NEAR1_CALLER, N - edge.size), edge]),)


def _sincos_inputs(seed=5):
    """the five sets of the sincos_step test as it stood, by name"""
    rng = np.random.default_rng(seed)
    return (("|x| <= pi (the Euler angles, latitude, longitude)", rng.uniform(-np.pi, np.pi, 400000)),
            ("|x| <= 1e3", rng.uniform(-1e3, 1e3, 400000)),
            ("|x| <= 1e6 (a heading wound up through 160 000 turns)", rng.uniform(-1e6, 1e6, 400000)),
            ("near the multiples of pi/2", np.concatenate([k * (np.pi / 2) + rng.uniform(-1e-6, 1e-6, 2000) for k in range(-40, 41)])),
            ("quadrant boundaries", np.concatenate([(k + 0.5) * (np.pi / 2) + rng.uniform(-1e-9, 1e-9, 500) for k in range(-40, 41)])))


def sincos_sets():
    return _cached("sincos_sets", lambda: tuple((name, np.ascontiguousarray(x)) for name, x in _sincos_inputs()))


def _half_angle_inputs(seed):
    rng = np.random.default_rng(seed)
    th, r = rng.uniform(-np.pi, np.pi, 500_000), _logu(rng, 1e-3, 1e3, 500_000)
    parts = [(r * np.sin(th), r * np.cos(th))]                                                 # all quadrants
    x = -_logu(rng, 1e-3, 1e3, 250_000)
    parts.append((-x * 10.0 ** -rng.uniform(0, 300, 250_000) * _sign(rng, 250_000), x))       # x < 0, y -> +-0: heading +-pi
    y = _logu(rng, 1e-3, 1e3, 150_000) * _sign(rng, 150_000)
    parts.append((y, np.abs(y) * 10.0 ** -rng.uniform(0, 300, 150_000) * _sign(rng, 150_000)))   # x -> 0
    return _fill(parts, N, lambda m: (rng.standard_normal(m), rng.standard_normal(m)))         # ... and unit-scale vectors


def _isa_inputs(seed):
    rng = np.random.default_rng(seed)
    edge = np.concatenate([np.array([hc, np.nextafter(hc, 0), np.nextafter(hc, np.inf)]) for hc in ISA_HC] + [np.array([0.0, -1000.0, 85000.0, 1e5])])
    near = np.concatenate([hc + rng.uniform(-1, 1, 2000) for hc in ISA_HC[:-1]] + [ISA_HC[-1] - rng.uniform(0, 1, 2000)])
    h = np.concatenate([np.tile(edge, 40), near, rng.uniform(*H_RANGE, 600_000)])
    h = np.concatenate([h, rng.uniform(-1000.0, 11000.0, N - h.size)])                        # the rest where aircraft fly
    T = rng.uniform(*T_SL_RANGE, N)
    T[::7] = rng.choice(np.array([T_SL_RANGE[0], 288.15, T_SL_RANGE[1]]), T[::7].size)
    return np.ascontiguousarray(h), np.ascontiguousarray(T)


# ---- long double references ----------------------------------------------------------------------------------------------------------------
def _ref_half_angle(y, x):
    """cos, sin of atan2(y, x) / 2 from the half-angle identities in long double, the square root always of a number >= 1/2 (evaluating
    the angle and halving it would lose the small component to the angle's own rounding)"""
    y, x = LD(1) * y, LD(1) * x
    r = np.hypot(x, y)
    big = np.sqrt((1 + np.abs(x) / r) / 2)
    small = np.abs(y) / (2 * r * big)
    return np.where(x >= 0, big, small), np.copysign(np.where(x >= 0, small, big), y)


def isa_layer(h):
    """index of the layer h lies in (7: at or above 84 852 m)"""
    return np.searchsorted(ISA_HC, h, side="right")


def _ref_isa(h, T_sl):
    """T, p / p_sl, log(p / p_sl) of the ISA in long double, the layer constants being the kernel's doubles"""
    h, T_sl = LD(1) * h, LD(1) * T_sl
    R, g = LD(ISA_R), LD(ISA_G)
    hb, Tb, lnp = np.zeros_like(h), T_sl.copy(), np.zeros_like(h)
    T = T_sl.copy()
    active = np.ones(h.shape, bool)
    for i in range(7):
        beta, hc = LD(ISA_BETA[i]), LD(ISA_HC[i])
        hh = np.minimum(h, hc)
        Tn = Tb + beta * (hh - hb)
        e = -g / (beta * R) * np.log1p(beta / Tb * (hh - hb)) if ISA_BETA[i] != 0 else -g / (R * Tb) * (hh - hb)
        T = np.where(active, Tn, T)
        lnp = np.where(active, lnp + e, lnp)
        active = active & (h >= hc)
        hb, Tb = np.full_like(h, hc), np.where(active, Tn, Tb)
    return T, np.exp(lnp), lnp


# Error count for isa_data, in units of 2^-52, per layer L = 0 .. 6 the altitude lies in (cumulative).
#   a layer with a lapse rate: e = c log(u), u = 1 + beta / Tb (hh - hb), |c| = g / (|beta| R) = 5.256, 34.163, 12.201, 12.201, 17.082.
#     u carries <= 1.57 (the quotient 1, the difference, the product and the sum 0.5 each, on |u - 1| <= 0.3 and u >= 0.7), the logarithm
#     <= 0.75 (3 ulp, or log_near1's 2.36, of a number below 0.5), the base temperature's own error <= 0.3: 3 |c| at the most; the
#     product's two roundings |e|, and the sum lnp += e half of |lnp|.
#   an isothermal layer: e = -g / (R Tb) (hh - hb): 3.5 |e| and half of |lnp|.
#   |e| and |lnp| at their largest, T_sl = 238.15 K: |e| = 1.88, 1.85, 2.38, 2.58, 0.62, 3.57, 3.15.
ISA_LNP_BOUND = np.array([18.0, 26.0, 134.0, 178.0, 185.0, 231.0, 294.0])      # |lnp - ref|            <= this * 2^-52
ISA_P_BOUND = ISA_LNP_BOUND + 3.5 * np.arange(1, 8)                            # |p - ref| / ref        <= this * 2^-52: exp 3 ulp and a product per layer
ISA_T_BOUND = np.arange(1, 8) * 1.0                                            # |T - ref|              <= this * 2^-44: 1 ulp of 256 .. 512 K per layer


def isa_errors(got, ref, h):
    """(T, p, lnp) errors of a run in units of their bounds' scales, and the bounds per point; points at or above 84 852 m are left out"""
    ok = h < ISA_HC[-1]
    L = isa_layer(h[ok])
    eT = abs_err(got[0][ok], ref[0][ok]) / 2.0 ** -44
    ep = (abs_err(got[1][ok], ref[1][ok]) / np.asarray(ref[1][ok], dtype=np.float64)) / 2.0 ** -52
    el = abs_err(got[2][ok], ref[2][ok]) / 2.0 ** -52
    return (eT, ep, el), (ISA_T_BOUND[L], ISA_P_BOUND[L], ISA_LNP_BOUND[L]), ok


# fp32 exp_step(x) = v_exp_f32(fl(x c)), c = fl32(log2 e), x in [-2, 0.2]: t = x c has |t| < 4, so its rounding is <= 2^-23, and |x| |c - log2 e|
# <= 2 * 1.8e-8; d(2^t) = ln2 2^t dt with 2^t <= e^0.2; the hardware function is 1 ulp of a result below 2: 2^-23.
EXP_STEP_RANGE = (-2.0, 0.2)
_C_EXP = float(np.float32(1.4426950408889634))
EXP_STEP_BOUND = 2.0 ** -23 + np.log(2.0) * np.exp(0.2) * (2.0 ** -23 + 2.0 * abs(_C_EXP - 1.4426950408889634))
# fp32 log_step(x) = fl(v_log_f32(x) k), k = fl32(ln 2), x in [0.69, 1.03]: |log2 x| <= 0.5354 < 1, so 1 ulp of the hardware function is <= 2^-24,
# scaled by ln 2; |log2 x| |k - ln 2|; the product is below 0.5: its rounding <= 2^-26.
LOG_STEP_RANGE = (0.69, 1.03)
_K_LOG = float(np.float32(0.6931471805599453))
LOG_STEP_BOUND = np.log(2.0) * 2.0 ** -24 + 0.5354 * abs(_K_LOG - 0.6931471805599453) + 2.0 ** -26


# fp32 atan2_fast: the source said "2e-7 absolute"; the host measures 3.5e-7 with a correctly rounded reciprocal (near +-pi one ulp is 2.4e-7),
# so the claim is corrected to this count, made before any device run (the source's comment now carries it):
#   first octant, a = t P(t^2), t = mn * rcp(mx):
#     the polynomial with its fp32 coefficients, in exact arithmetic     1.10e-7   (ATAN2_FAST_POLY; the host test recomputes it)
#     t: 1 ulp of v_rcp_f32 and the product's rounding, through dt/(1+t^2) with t/(1+t^2) <= 1/2      0.5 (2^-23 + 2^-24)
#     s = t t, the Horner steps and the last product, on a <= pi/4                                   2^-25 + 2^-24 pi/4 + 2^-25 pi/4
#   pi/2 - a (|y| > |x|):   |fl32(pi/2) - pi/2| = 4.4e-8 and half an ulp of a result below 2        2^-24
#   pi - a   (x < 0):       |fl32(pi) - pi|     = 8.7e-8 and half an ulp of a result below 4        2^-23
ATAN2_FAST_POLY = 1.10e-7
ATAN2_FAST_OCTANT = ATAN2_FAST_POLY + 0.5 * (2.0 ** -23 + 2.0 ** -24) + 2.0 ** -25 + (2.0 ** -24 + 2.0 ** -25) * np.pi / 4
ATAN2_FAST_XPOS_BOUND = ATAN2_FAST_OCTANT + abs(HALF_PI_F - np.pi / 2) + 2.0 ** -24
ATAN2_FAST_BOUND = ATAN2_FAST_XPOS_BOUND + abs(PI_F - np.pi) + 2.0 ** -23
def atan2_fast_bounds(y, x):
    """the count above, per point: each region is held to its own figure (3.0e-7 in the first octant, 4.0e-7 after pi/2 - a alone,
    5.1e-7 after pi - a alone, 6.1e-7 after both)"""
    b = np.full(y.shape, ATAN2_FAST_OCTANT)
    b[np.abs(y) > np.abs(x)] += abs(HALF_PI_F - np.pi / 2) + 2.0 ** -24
    b[x < 0] += abs(PI_F - np.pi) + 2.0 ** -23
    return b


ATAN2_FAST_COEF =(-0.00478042708709836, 0.024557026103138924, -0.05990458279848099, 0.09942749887704849, -0.1402941644191742, 0.19971375167369843,
                   -0.3333209455013275, 0.9999999403953552)   # (as in the source; the host test checks that they still are)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """op: the FB_MP_* name; inputs() -> (a,) or (a, b); ref(a[, b]) -> tuple of long double arrays, one per output; measure "ulp" | "abs";
    mant 52 | 23; claim: the source's figure (None: it states none); H: the host worst case, recorded (None: not measurable on the host);
    ndiv: fp64 divisions on the path; fixed: a bound that does not follow the H rule (division, fp32, the library), with its reason above"""
    def __init__(self, op, inputs, ref, domain, measure="ulp", mant=52, claim=None, H=None, ndiv=0, fixed=None, regions=None):
        self.op, self._inputs, self._ref, self.domain = op, inputs, ref, domain
        self.regions = regions     # (inputs) -> a bound per point, where parts of the domain have tighter counts than `bound` (their maximum)
        self.measure, self.mant, self.claim, self.H, self.ndiv, self.fixed = measure, mant, claim, H, ndiv, fixed

    def inputs(self):
        return _cached(("in", self.op), lambda: tuple(self._inputs()))

    def ref(self):
        return _cached(("ref", self.op), lambda: tuple(np.asarray(r, dtype=LD) for r in self._ref(*self.inputs())))

    def errors(self, outs):
        f = (lambda g, r: ulps(g, r, self.mant)) if self.measure == "ulp" else abs_err
        return tuple(f(g, r) for g, r in zip(outs, self.ref()))

    def within(self, errs):
        """every point inside its bound (the per-point one where the case has regions)"""
        b = self.regions(*self.inputs()) if self.regions else self.bound
        return all(bool((e <= b).all()) for e in errs)

    @property
    def bound(self):
        if self.fixed is not None:
            return self.fixed
        assert self.H is not None
        return max(self.claim or 0.0, self.H + 0.5 * self.ndiv)


_ld = lambda a: LD(1) * a
_sc = lambda x: (np.sin(_ld(x)), np.cos(_ld(x)))
_sincos_all = lambda: (np.ascontiguousarray(np.concatenate([x for _, x in sincos_sets()])),)
_f32 = lambda a: np.ascontiguousarray(a.astype(np.float32).astype(np.float64))

# H: tests/test_math_primitives_host.py measures it (contraction off / on) and asserts that the record below still covers what it measures.
CASES = {c.op: c for c in (
    Case("FB_MP_SQRT", lambda: _sqrt_inputs(11), lambda x: (np.sqrt(_ld(x)),), "[1e-280, 1e300]; 0 -> 0; below 1e-290: a number below 1e-145", claim=1.0, H=0.51),
    Case("FB_MP_RSQRT", lambda: _sqrt_inputs(12), lambda x: (1 / np.sqrt(_ld(x)),), "[1e-280, 1e300]", claim=1.0, H=1.0),
    Case("FB_MP_DIV", lambda: _div_inputs(13), lambda a, b: (_ld(a) / _ld(b),), "|a|, |b| in [2^-300, 2^301), so a / b in 2^+-601", fixed=1.0),
    Case("FB_MP_RCP", lambda: (_div_inputs(13)[1],), lambda x: (1 / _ld(x),), "x in 2^+-300", fixed=1.0),
    Case("FB_MP_HALF_ANGLE", lambda: _half_angle_inputs(14), _ref_half_angle, "x^2 + y^2 neither overflows nor underflows; (0, 0) -> (1, 0)", H=3.36),
    Case("FB_MP_ATAN2_TAB", lambda: _atan2_inputs(15), lambda y, x: (np.arctan2(_ld(y), _ld(x)),), "max(|x|, |y|) in [1e-30, 1e30], or x = y = 0", claim=1.6, H=2.07, ndiv=1),
    Case("FB_MP_ATAN2_TAB_XPOS", lambda: _atan2_inputs(16, xpos=True), lambda y, x: (np.arctan2(_ld(y), _ld(x)),), "x >= 0, max(x, |y|) in [1e-30, 1e30]", claim=1.6, H=1.81, ndiv=1),
    Case("FB_MP_LOG_NEAR1", lambda: _log_near1_inputs(17), lambda u: (np.log1p(_ld(u) - 1),), "[0.65, 1.5]; the caller's range is [0.6997, 1.03]", claim=1.5, H=1.93, ndiv=1),
    Case("FB_MP_SINCOS_STEP", _sincos_all, _sc, "|x| < 1e6", claim=1.5, H=1.48),
    Case("FB_MP_LIB_EXP", lambda: (np.random.default_rng(18).uniform(-40.0, 40.0, N),), lambda x: (np.exp(_ld(x)),), "[-40, 40]", fixed=3.0),
    Case("FB_MP_LIB_LOG", lambda: (np.concatenate([_logu(np.random.default_rng(19), 1e-300, 1e300, N // 2), _log_near1_inputs(19)[0][:N - N // 2]]),),
         lambda x: (np.log(_ld(x)),), "[1e-300, 1e300]", fixed=3.0),
    Case("FB_MP_LIB_SINCOS", _sincos_all, _sc, "|x| < 1e6", fixed=4.0),
    Case("FB_MP_LIB_ATAN2", lambda: _atan2_inputs(15), lambda y, x: (np.arctan2(_ld(y), _ld(x)),), "as atan2_tab", fixed=6.0),
    Case("FB_MP_F32_ATAN2_FAST", lambda: _atan2_inputs(20, f32=True), lambda y, x: (np.arctan2(_ld(y), _ld(x)),), "max(|x|, |y|) in [1e-30, 1e30], or x = y = 0",
         measure="abs", mant=23, claim=ATAN2_FAST_BOUND, fixed=ATAN2_FAST_BOUND, regions=atan2_fast_bounds),
    Case("FB_MP_F32_ATAN2_FAST_XPOS", lambda: _atan2_inputs(21, f32=True, xpos=True), lambda y, x: (np.arctan2(_ld(y), _ld(x)),), "x >= 0, max(x, |y|) in [1e-30, 1e30]",
         measure="abs", mant=23, claim=ATAN2_FAST_XPOS_BOUND, fixed=ATAN2_FAST_XPOS_BOUND, regions=atan2_fast_bounds),
    Case("FB_MP_F32_EXP_STEP", lambda: (_f32(np.concatenate([np.random.default_rng(22).uniform(*EXP_STEP_RANGE, N - 14), 10.0 ** -np.arange(1, 8), -10.0 ** -np.arange(1, 8)])),),
         lambda x: (np.exp(_ld(x)),), "[-2, 0.2]: the ISA's use", measure="abs", mant=23, fixed=EXP_STEP_BOUND),
    Case("FB_MP_F32_LOG_STEP", lambda: (_f32(np.concatenate([np.random.default_rng(23).uniform(*LOG_STEP_RANGE, N - 14), 1 - 10.0 ** -np.arange(1, 8), 1 + 10.0 ** -np.arange(2, 9)])),),
         lambda x: (np.log(_ld(x)),), "[0.69, 1.03]: the ISA's use", measure="abs", mant=23, fixed=LOG_STEP_BOUND),
    Case("FB_MP_F32_SQRT", lambda: _sqrt_inputs(24, f32=True), lambda x: (np.sqrt(_ld(x)),), "[1e-37, 1e38]", mant=23, claim=2.5, fixed=2.5),
    Case("FB_MP_F32_RSQRT", lambda: _sqrt_inputs(25, f32=True), lambda x: (1 / np.sqrt(_ld(x)),), "[1e-37, 1e38]", mant=23, fixed=2.0),   # (OpenCL's limit for rsqrt; the source states none)
    Case("FB_MP_F32_DIV", lambda: _div_inputs(26, f32=True), lambda a, b: (_ld(a) / _ld(b),), "a, b in 2^+-60", mant=23, claim=2.5, fixed=2.5),
)}
ISA_OPS = ("FB_MP_ISA_FAST", "FB_MP_ISA")
SEEDED_OPS = ("FB_MP_SQRT", "FB_MP_RSQRT", "FB_MP_HALF_ANGLE")   # built on v_rsq_f64: their H is the worst over the host's seed runs (test_seed_sensitivity)
HOST_OPS = tuple(op for op, c in CASES.items() if not op.startswith("FB_MP_LIB_") and op not in ("FB_MP_DIV", "FB_MP_RCP", "FB_MP_F32_DIV", "FB_MP_F32_SQRT", "FB_MP_F32_RSQRT"))


def isa_inputs():
    return _cached("isa_in", lambda: _isa_inputs(27))


def isa_ref():
    return _cached("isa_ref", lambda: _ref_isa(*isa_inputs()))


def table_ref():
    return _cached("table", lambda: np.arctan(LD(1) * np.arange(33) / 32))


# ---- special values: behaviour, not accuracy ------------------------------------------------------------------------------------------------
# (op, a, b, expected out0, expected out1 or None, tol). tol 0: the same bits (NaN for NaN, the zero's sign included); tol > 0: within tol;
# an expected (lo, hi) pair: inside the interval. "source": the primitive's comment says so; "does": the source is silent and this is what the
# host transcription returns, recorded so that a change shows (the comment now carries the domain that excludes it).
NAN, INF = float("nan"), float("inf")
SERIES_AT_1 = 1 - 1 / 3 + 1 / 5 - 1 / 7 + 1 / 9     # atan2_tab outside its domain: entry 0 and the four-term series summed at r = 1
SPECIALS = (
    ("FB_MP_ATAN2_TAB", 0.0, 0.0, 0.0, None, 0, "source: atan2(0, 0) = 0"),
    ("FB_MP_ATAN2_TAB", -0.0, 0.0, -0.0, None, 0, "source: ... with the sign of y"),
    ("FB_MP_ATAN2_TAB", 0.0, -0.0, 0.0, None, 0, "source: the sign of a zero x is not examined"),
    ("FB_MP_ATAN2_TAB", 0.0, -1.0, PI_D, None, 0, "source"),
    ("FB_MP_ATAN2_TAB", -0.0, -1.0, -PI_D, None, 0, "source"),
    ("FB_MP_ATAN2_TAB", 0.0, 1.0, 0.0, None, 0, "source"),
    ("FB_MP_ATAN2_TAB", -0.0, 1.0, -0.0, None, 0, "source"),
    ("FB_MP_ATAN2_TAB", 1.0, 0.0, HALF_PI_D, None, 0, "source"),
    ("FB_MP_ATAN2_TAB", -1.0, -0.0, -HALF_PI_D, None, 0, "source"),
    ("FB_MP_ATAN2_TAB", NAN, 1.0, PI_D / 4, None, 1e-15, "does: fmax / fmin drop the NaN"),
    ("FB_MP_ATAN2_TAB", 1.0, NAN, PI_D / 4, None, 1e-15, "does"),
    ("FB_MP_ATAN2_TAB", NAN, NAN, 0.0, None, 1e-300, "does: the guard mx > 0 fails and gives atan2(0, 0)'s answer"),
    ("FB_MP_ATAN2_TAB", INF, 1.0, NAN, None, 0, "does: t_i mx = 0 inf (the library: pi/2)"),
    ("FB_MP_ATAN2_TAB", -INF, 1.0, NAN, None, 0, "does (the library: -pi/2)"),
    ("FB_MP_ATAN2_TAB", 1.0, INF, NAN, None, 0, "does (the library: 0)"),
    ("FB_MP_ATAN2_TAB", 1.0, -INF, NAN, None, 0, "does (the library: pi)"),
    ("FB_MP_ATAN2_TAB", INF, INF, NAN, None, 0, "does (the library: pi/4)"),
    ("FB_MP_ATAN2_TAB", 1e-300, 1e-300, SERIES_AT_1, None, 1e-12, "does: outside the domain, not pi/4"),
    ("FB_MP_ATAN2_TAB", 1e300, 1e300, SERIES_AT_1, None, 1e-12, "does: outside the domain, not pi/4"),
    # fp32-denormal magnitudes: the estimate is infinite (denormals kept: a denormal times the infinite reciprocal of one) or NaN (flushed);
    # the clamped index selects entry 32 (r = 0: pi/4, the right answer by luck) or entry 0 (the series at r = 1): bounded either way
    ("FB_MP_ATAN2_TAB", 1e-40, 1e-40, (PI_D / 4 - 1e-15, SERIES_AT_1 + 1e-12), None, 0, "does: outside the domain, wrong but bounded"),
    ("FB_MP_ATAN2_TAB_XPOS", 1e-40, 1e-40, (PI_D / 4 - 1e-15, SERIES_AT_1 + 1e-12), None, 0, "does: outside the domain, wrong but bounded"),
    ("FB_MP_ATAN2_TAB", -1e-40, -3e-40, (-PI_D, -HALF_PI_D), None, 0, "does: outside the domain; the quadrant holds"),
    ("FB_MP_ATAN2_TAB", 1e-40, 1.0, 1e-40, None, 1e-54, "source: mn an fp32 denormal next to a normal mx is INSIDE the domain (entry 0, r = mn / mx)"),
    ("FB_MP_ATAN2_TAB_XPOS", 1e-40, 1.0, 1e-40, None, 1e-54, "source: the same"),
    ("FB_MP_ATAN2_TAB", 1.0, -1e-40, HALF_PI_D, None, 1e-15, "source: the same, next to pi/2"),
    ("FB_MP_ATAN2_TAB_XPOS", 1.0, 0.0, HALF_PI_D, None, 0, "source"),
    ("FB_MP_ATAN2_TAB_XPOS", 0.0, 1.0, 0.0, None, 0, "source"),
    ("FB_MP_ATAN2_TAB_XPOS", -0.0, 1.0, -0.0, None, 0, "source"),
    ("FB_MP_SQRT", 0.0, None, 0.0, None, 0, "source: 0 -> 0"),
    ("FB_MP_SQRT", -0.0, None, -0.0, None, 0, "source: as sqrt()"),
    ("FB_MP_SQRT", NAN, None, NAN, None, 0, "source: NaN -> NaN"),
    ("FB_MP_SQRT", 1e-291, None, (0.0, 1e-145), None, 0, "source: below 1e-290 treated as 0 (a number below sqrt(1e-290))"),
    ("FB_MP_SQRT", 1e-300, None, (0.0, 1e-145), None, 0, "source"),
    ("FB_MP_SQRT", 5e-324, None, (0.0, 1e-145), None, 0, "source"),
    ("FB_MP_SQRT", INF, None, NAN, None, 0, "does (the library: inf)"),
    ("FB_MP_RSQRT", NAN, None, NAN, None, 0, "does"),
    ("FB_MP_RSQRT", 0.0, None, NAN, None, 0, "does: x > 0 (the library: inf)"),
    ("FB_MP_RSQRT", INF, None, NAN, None, 0, "does (the library: 0)"),
    ("FB_MP_HALF_ANGLE", 0.0, 0.0, 1.0, 0.0, 0, "source: atan2(0, 0) = 0"),
    ("FB_MP_HALF_ANGLE", 0.0, -1.0, 0.0, 1.0, 0, "source: heading pi"),
    ("FB_MP_HALF_ANGLE", -0.0, -1.0, 0.0, -1.0, 0, "source: heading -pi"),
    ("FB_MP_HALF_ANGLE", 0.0, 1.0, 1.0, 0.0, 0, "source"),
    ("FB_MP_HALF_ANGLE", -0.0, 1.0, 1.0, -0.0, 0, "source"),
    ("FB_MP_HALF_ANGLE", NAN, 1.0, 1.0, 0.0, 0, "does: a NaN fails r2 > 0 and takes the (0, 0) answer"),
    ("FB_MP_HALF_ANGLE", INF, 1.0, NAN, NAN, 0, "does"),
    ("FB_MP_LOG_NEAR1", 1.0, None, 0.0, None, 0, "source"),
    ("FB_MP_LOG_NEAR1", NAN, None, NAN, None, 0, "does"),
    ("FB_MP_SINCOS_STEP", 0.0, None, 0.0, 1.0, 0, "source"),
    ("FB_MP_SINCOS_STEP", NAN, None, NAN, NAN, 0, "source: NaN and inf give NaN like the library"),
    ("FB_MP_SINCOS_STEP", INF, None, NAN, NAN, 0, "source"),
    ("FB_MP_SINCOS_STEP", -INF, None, NAN, NAN, 0, "source"),
    ("FB_MP_DIV", NAN, 1.0, NAN, None, 0, "IEEE"),
    ("FB_MP_DIV", 1.0, NAN, NAN, None, 0, "IEEE"),
    ("FB_MP_DIV", 0.0, 3.0, 0.0, None, 0, "IEEE"),
    ("FB_MP_F32_ATAN2_FAST", 0.0, 0.0, 0.0, None, 0, "source: atan2(0, 0) = 0"),
    ("FB_MP_F32_ATAN2_FAST", 0.0, -1.0, PI_F, None, 0, "source"),
    ("FB_MP_F32_ATAN2_FAST", -0.0, -1.0, -PI_F, None, 0, "source"),
    ("FB_MP_F32_ATAN2_FAST", 0.0, 1.0, 0.0, None, 0, "source"),
    ("FB_MP_F32_ATAN2_FAST", 1.0, 0.0, HALF_PI_F, None, 0, "source"),
    ("FB_MP_F32_ATAN2_FAST", NAN, 1.0, PI_D / 4, None, 2e-7, "does: fmaxf / fminf drop the NaN"),
    ("FB_MP_F32_ATAN2_FAST", INF, 1.0, HALF_PI_F, None, 0, "does"),
    ("FB_MP_F32_EXP_STEP", 0.0, None, 1.0, None, 2.0 ** -23, "1 ulp of the hardware function"),
    ("FB_MP_F32_EXP_STEP", NAN, None, NAN, None, 0, "does"),
    ("FB_MP_F32_LOG_STEP", 1.0, None, 0.0, None, 2.0 ** -24, "1 ulp of the hardware function"),
    ("FB_MP_F32_LOG_STEP", NAN, None, NAN, None, 0, "does"),
)


def special_ok(got, want, tol):
    if isinstance(want, tuple):
        return want[0] <= got <= want[1]
    if np.isnan(want):
        return bool(np.isnan(got))
    if tol == 0:
        return got == want and np.signbit(got) == np.signbit(want)
    return abs(got - want) <= tol


def check_specials(run, ops=None):
    """run(op, a, b) -> (out0, out1): arrays for arrays. Returns the list of failures (empty: the table holds)."""
    bad = []
    for op, a, b, w0, w1, tol, why in SPECIALS:
        if ops is not None and op not in ops:
            continue
        o0, o1 = run(op, np.array([a]), None if b is None else np.array([b]))
        if not special_ok(float(o0[0]), w0, tol) or (w1 is not None and not special_ok(float(o1[0]), w1, tol)):
            bad.append((op, a, b, "got", float(o0[0]), None if w1 is None else float(o1[0]), "want", w0, w1, why))
    return bad
