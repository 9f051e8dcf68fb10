// c172_device_impl.inc — body of c172_device.hpp, written once over the arithmetic type `real` and instantiated by that header
// for double (namespace fbd: the parity path) and float (namespace fbf: the fp32 airborne stepper). FBL(x) casts a literal
// to `real` at compile time. Not a stand-alone header.
namespace FB_NS {
typedef FB_REAL real;


#define FBD __device__ __forceinline__
// Marks the phase boundaries of one RHS. It used to be a scheduling barrier (__builtin_amdgcn_sched_barrier(0)): while the kernel
// sat at the register limit, letting the scheduler interleave the phases cost more in spills than the ILP gained. Since the
// instruction diet of DESIGN.md v9-v15 the registers have slack and the barrier costs 1 %, so it is off.
// FB_STAMP (diagnostic builds only, tools/stamp_profile.py): every fence reads the shader clock and wave 0 of workgroup 0 adds
// the cycles since the previous fence to g_stamp_acc[k] — a per-phase cycle profile of one wave (MI355X_MICROARCH.md: in-kernel stamps).
#if defined(FB_STAMP) || defined(FB_TRIM_STAMP)
__device__ unsigned long long g_stamp_acc[32], g_stamp_cnt[32], g_stamp_last;
#endif
#ifdef FB_STAMP
__device__ __forceinline__ void fb_stamp(int k) {
    __builtin_amdgcn_sched_barrier(0);
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        __builtin_amdgcn_s_waitcnt(0);   // drain: what is still in flight belongs to the phase that issued it
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (threadIdx.x == 0) { g_stamp_acc[k] += t - g_stamp_last; g_stamp_cnt[k] += 1; }
        __threadfence();
        __builtin_amdgcn_s_waitcnt(0);
        if (threadIdx.x == 0) g_stamp_last = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_waitcnt(0);
    }
    __builtin_amdgcn_sched_barrier(0);
}
#endif
#if defined(FB_PHASE_MARK)   // diagnostic: "; FBPHASE k" comments in the device assembly, for per-phase instruction counts (tools/phase_mix.py)
#define PHASE_FENCE(k) asm volatile("; FBPHASE %0" ::"n"(k) : "memory")
#elif defined(FB_STAMP)
#define PHASE_FENCE(k) fb_stamp(k)
#else
#define PHASE_FENCE(k) do { } while (0)
#endif
constexpr int SCALAR_KNOTS_MIN = 3;   // tables with at most this many knots are scanned from LDS even when the scalar path is on
// The ground-contact branch of a landing-gear unit is INLINED into the kernels that can meet the ground (k_step_air<.., true>, k_f_ode,
// k_f_step, k_trim). It used to be out of line, when the airborne and the ground-capable stepper were one kernel and the airborne
// path could not afford its registers; since the airborne pass is a kernel of its own (GROUND = false: the branch is compiled out)
// the call only cost the ground-capable pass its stack frame — GroundIn / GroundOut through scratch memory at every contact:
// 5.1e8 -> 9.4e8 aircraft-steps/s for a batch that sits on the ground (tools/bench_ground.py).

constexpr real PI = FBL(3.14159265358979323846);

// ---- resident-capable constants -----------------------------------------------------------------------------------------------------
// gfx950's VOP3 encoding takes no fp64 literal: an fp64 constant that is no inline constant is a register pair built by two moves, at
// every use (the build runs without machine LICM, and why: __graft_entry__.py). A kernel that HAS registers to spare — role P of
// k_step_duo, c172_kernels.hpp — keeps such constants resident for the whole launch instead. So the helpers below take their constants
// from a PROVIDER, kc<ID>(K): the default provider KLit returns the literal KC<ID>::v and every caller that passes none compiles as it
// always did; a resident provider (DuoK, c172_kernels.hpp) returns a register for the first NK ids and the literal for the rest.
// THE ORDER OF THE IDS IS THE PRIORITY (moves saved per register pair, counted on the assembly by tools/loop_literals.py): first the
// constants used at several inlined sites, then the series coefficients and unit factors of the straight-line path; constants that
// appear only in rare branches (the ISA layers above 11 km, the library exp) are no ids at all. A value is defined ONCE, here, by the
// expression the compiler folded at the use before (e.g. the reciprocal that -freciprocal-math makes of a division by a constant).
enum {
    // atan2_tab (four inlined sites in role P: latitude, longitude, the propeller's two flow angles), geoid_height
    KC_AT_C3, KC_AT_C5, KC_AT_C7, KC_AT_C9, KC_HALF_PI, KC_TWO_PI, KC_PI, KC_GEOID_PER_RAD,
    KC_SQRT_TINY,   // sqrt(): three sites (the geoid's cos(lat), the propeller's airspeed and its in-plane component)
    // isa_data<true>: the troposphere, straight-line
    KC_ISA_H11, KC_ISA_BETA0, KC_ISA_LNP, KC_ISA_CFRAC,
    KC_LN_C3, KC_LN_C5, KC_LN_C7, KC_LN_C9, KC_LN_C11, KC_LN_C13, KC_LN_C15, KC_LN_C17, KC_LN_C19, KC_LN_C21,
    KC_EXP_C3, KC_EXP_C4, KC_EXP_C5, KC_EXP_C6, KC_EXP_C7, KC_EXP_C8, KC_EXP_C9,
    KC_HELPERS_END   // (the ids of rhs_duo's own constants follow: c172_duo_device.hpp)
};
template <int I> struct KC;
#define FB_KC(id, expr) template <> struct KC<id> { static constexpr real v = (expr); }
// ... and a constant the source DIVIDES by, which -freciprocal-math turns into a multiplication by the reciprocal: the resident value is
// that reciprocal, x * (1 / den); the literal provider keeps the division as written, so that such a caller's code is what it always was
#define FB_KC_RCP(id, expr) template <> struct KC<id> { static constexpr real den = (expr), v = 1 / den; }
struct KLit {
    template <int I> static constexpr bool resident() { return false; }
    template <int I> FBD constexpr real get() const { return KC<I>::v; }
};
template <int I, class KP> FBD real kc(const KP& K) { return K.template get<I>(); }
template <int I, class KP> FBD real kc_div(real x, const KP& K) {
    if constexpr (KP::template resident<I>()) return x * K.template get<I>(); else return x / KC<I>::den;
}
FB_KC(KC_AT_C3, -1.0 / 3); FB_KC(KC_AT_C5, 1.0 / 5); FB_KC(KC_AT_C7, -1.0 / 7); FB_KC(KC_AT_C9, 1.0 / 9);
FB_KC(KC_HALF_PI, FBL(1.5707963267948966)); FB_KC(KC_TWO_PI, 2 * PI); FB_KC(KC_PI, FBL(3.141592653589793));
FB_KC(KC_GEOID_PER_RAD, 720 / PI);   // EGM96 grid cells per radian, both axes
FB_KC(KC_SQRT_TINY, sizeof(real) == 8 ? 1e-290 : 0.0);   // (the fp64 form's floor; the fp32 form is the library's)
static_assert(KC<KC_HALF_PI>::v == PI / 2 && KC<KC_GEOID_PER_RAD>::v == 1440 / (2 * PI), "one constant serves both uses");

// fp64 square roots without the library's range scaling and special-case fix-up (9 instructions instead of 17; at one wave per
// SIMD every instruction costs an issue slot): v_rsq_f64 seed, one coupled Goldschmidt step on (g ~ sqrt x, h ~ 1/(2 sqrt x))
// and one residual correction -> <= 1 ulp (measured: 0.50 ulp on the host whatever the seed's error up to 2^-23; the device's figure
// is in docs/design/k_step_air.md, "Math primitives, measured", like every figure below). Arguments here are sums of squares and
// physical magnitudes. DOMAIN [1e-280, 1e300]; 0 and NaN behave as in sqrt() (0 -> 0, NaN -> NaN); numbers below 1e-290 are treated
// as 0 (the result is some number below 1e-145); +inf gives NaN (the seed is 0), unlike sqrt().
template <class KP = KLit>
FBD real sqrt(real x, const KP& K = KP{}) {
    if constexpr (sizeof(real) == 8) {
        const double y = __builtin_amdgcn_rsq(__builtin_fmax((double)x, (double)kc<KC_SQRT_TINY>(K)));
        double g = x * y, h = 0.5 * y;
        const double r = __builtin_fma(-h, g, 0.5);
        g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
        return __builtin_fma(__builtin_fma(-g, g, x), h, g);
    } else {
        return ::sqrtf(x);
    }
}
// <= 1 ulp: 0.74 ulp on the host with a correctly rounded seed, 1.00 with any other (seed error up to 2^-23). x = 0 and x = +inf give NaN.
FBD real rsqrt(real x) {   // x > 0, finite: [1e-280, 1e300] is tested
    if constexpr (sizeof(real) == 8) {
        double y = __builtin_amdgcn_rsq((double)x);
        double r = __builtin_fma(-0.5 * y, x * y, 0.5);
        y = __builtin_fma(y, r, y);
        r = __builtin_fma(-0.5 * y, x * y, 0.5);
        return __builtin_fma(y, r, y);
    } else {
        return ::rsqrtf(x);
    }
}

// ---------------------------------------------------------------------------------------------
// small vector / quaternion algebra (FlightPhysics/src/quaternions.jl:109-115; attitude.jl:93-118)
struct v3 { real x, y, z; };
FBD v3 operator+(v3 a, v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
FBD v3 operator-(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
FBD v3 operator-(v3 a) { return {-a.x, -a.y, -a.z}; }
FBD v3 operator*(real s, v3 a) { return {s * a.x, s * a.y, s * a.z}; }
FBD real dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
FBD v3 cross(v3 a, v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
template <class KP = KLit>
FBD real norm(v3 a, const KP& K = KP{}) { return sqrt(dot(a, a), K); }

struct quat { real w, x, y, z; };
FBD quat qmul(quat a, quat b) {
    return {a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z),
            a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y),
            a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z),
            a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x)};
}
FBD quat qconj(quat q) { return {q.w, -q.x, -q.y, -q.z}; }
// v' = v + 2 q_im x (q_re v + q_im x v)   (attitude.jl:98-103)
FBD v3 qrot(quat q, v3 v) {
    const v3 qi = {q.x, q.y, q.z};
    const v3 t = q.w * v + cross(qi, v);
    return v + cross(FBL(2.0) * qi, t);
}
FBD v3 qrot_inv(quat q, v3 v) { return qrot(qconj(q), v); }

// ---------------------------------------------------------------------------------------------
// WGS-84 (FlightPhysics/src/geodesy.jl:15-35)
namespace wgs {
constexpr real GM = FBL(3.986005e+14);
constexpr real a = FBL(6378137.0);
constexpr real f = 1 / FBL(298.257223563);
constexpr real w_ie = FBL(7.292115e-05);
constexpr real b = a * (1 - f);
constexpr real e2 = 2 * f - f * f;
constexpr real a2 = a * a;
constexpr real m = w_ie * w_ie * a * a * b / GM;
constexpr real g_a = FBL(9.7803253359);
constexpr real g_b = FBL(9.8321849378);
constexpr real k_g = b * g_b / (a * g_a) - 1;
}  // namespace wgs
constexpr real H_MIN = -FBL(1000.0);

// LDS pointers carry their address space: a generic `double*` into LDS compiles to flat_load/flat_store, whose
// LDS aperture only reaches the first 64 KB of a workgroup's allocation on gfx950 (measured: panels above that
// read back garbage through generic pointers) and which is slower than ds_read/ds_write anyway.
typedef __attribute__((address_space(3))) const real* lds_cptr;
typedef __attribute__((address_space(3))) real* lds_ptr;
typedef __attribute__((address_space(4))) const real* gk_cptr;   // read-only global memory (a copy of the blob in `real`), constant address space
struct Tables {
    lds_cptr lds;        // [aero | piston | propeller] blob in LDS
    const float* egm96;  // 721 x 1441 float32, column-major [lat, lon], global memory
    lds_cptr rk;         // rk[j] = 1 / (lds[j+1] - lds[j]) over the aero|piston part: reciprocal knot spacings
    gk_cptr gk;          // the same blob in global memory (in `real`), viewed through the CONSTANT address space: knot scans read it with
                         // uniform addresses, which the compiler then selects as scalar loads (s_load -> SGPRs, compared straight
                         // from there) instead of spending an LDS read and a VGPR pair per knot
};
constexpr int LDS_RK_KNOTS = AT_SIZE + PT_SIZE;     // reciprocal knot spacings, one slot per blob position
constexpr int LDS_ATAN = LDS_RK_KNOTS, ATAN_N = 33;   // behind them: atan(k / 32), k = 0..32, for atan2_tab()
constexpr int LDS_RK_DOUBLES = LDS_RK_KNOTS + 40;

// cos and sin of atan2(y, x) / 2 without evaluating the angle: half-angle identities arranged so that the
// square root is always taken of a number >= 1/2 (no cancellation). Used for the z- and y-rotation quaternions
// of the local-level frames, where only cos(angle/2), sin(angle/2) are needed (attitude.jl:288-308).
// Two rsqrt deep: <= 3.36 ulp on either output (host, seed error up to 2^-23; 2.92 with a correctly rounded seed). DOMAIN: x^2 + y^2
// neither overflows nor underflows, or x = y = 0. A NaN argument fails r2 > 0 and returns (1, 0) like (0, 0); an infinite one gives NaN.
FBD void half_angle_cs(real y, real x, real& c, real& s) {
    // branch-free: with cx = x/r, sy = y/r and h = (1 + |cx|)/2 >= 1/2, t = sqrt h is the larger of |cos|, |sin| of the half angle and
    // w = |sy| / (2 t) the smaller; which is which depends on the sign of x. One rsqrt gives both t = h rs and 1/t = rs.
    const real r2 = x * x + y * y;
    const bool ok = r2 > 0;
    const real ir = rsqrt(ok ? r2 : FBL(1.0));
    const real cx = x * ir, sy = y * ir;
    const real h = FBL(0.5) + FBL(0.5) * fabs(cx);
    const real rs = rsqrt(h);
    const real t = h * rs, w = (FBL(0.5) * fabs(sy)) * rs;
    const bool fwd = x >= 0;
    c = ok ? (fwd ? t : w) : FBL(1.0);                       // atan2(0, 0) = 0
    s = ok ? copysign(fwd ? w : t, y) : FBL(0.0);
}

// atan2 with one division: the octant's quotient t = min/max in [0, 1] is located on a 1/32 grid from a single-precision estimate,
// atan t = atan t_i + atan r with r = (min - t_i max) / (max + t_i min), |r| <= 1/64, so that four series terms reach 1e-19; atan t_i
// comes from a 33-entry table in LDS (tab). 53 instructions against the library's 70 (whose own polynomial needs 20 constants,
// two s_mov each). Error: 2.07 ulp on the host with a correctly rounded division (worst where the quotient changes table entry just
// below a power of two, y/x ~ 1/64; "<= 1.6" stood here unmeasured), <= 2.57 ulp with the device's 1-ulp division.
// atan2(0, 0) = 0; the sign of a zero x is not examined (atan2(0, -0) = 0, not π).
// DOMAIN: 1e-30 <= max(|x|, |y|) <= 1e30, or x = y = 0: the estimate is formed in single precision, and outside fp32's normal range it
// is NaN or infinite — (1e-300, 1e-300) and (1e300, 1e300) select entry 0 and return 0.8349, not π/4; at fp32-denormal magnitudes
// (1e-40, 1e-40) the estimate is NaN or infinite depending on how the denormals are treated, and the entry is 0 or (the index is
// clamped) 32: the result is WRONG BUT BOUNDED there, an angle of the right sign within [0, π], and every read stays inside the table.
// The call sites and their ranges are listed in docs/design/k_step_air.md: every one stays inside the domain for any state the
// integrator can reach; a state SET with two components both in (0, 1e-30) next to a guard that looks at a third does not.
// NaN does NOT come through: fmax / fmin drop it (atan2_tab(NaN, 1) = π/4, atan2_tab(NaN, NaN) = 0), so no caller may rely on this
// function to carry a NaN state forward (none does: the norms and sums next to every call carry it). An infinite argument gives NaN.
// XPOS: the caller guarantees x >= 0 and (x, y) != (0, 0) (x is a norm next to a non-zero y, or the cosine of a latitude): the
// x < 0 reflection and the atan2(0, 0) guard drop out.
template <bool XPOS = false, class KP = KLit>
FBD double atan2_tab(double y, double x, lds_cptr tab, const KP& K = KP{}) {
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const double mx = __builtin_fmax(ax, ay), mn = __builtin_fmin(ax, ay);
    const int i0 = (int)__builtin_rintf(((float)mn * __builtin_amdgcn_rcpf((float)mx)) * 32.0f);   // (NaN -> 0; never negative)
    const int i = i0 < ATAN_N - 1 ? i0 : ATAN_N - 1;   // in the domain i0 <= 32 already; outside it (an infinite estimate) the read stays in the table
    const double ti = (double)i * (1.0 / 32);
    const double r = (mn - ti * mx) / (mx + ti * mn), s = r * r;
    double p = __builtin_fma(s, (double)kc<KC_AT_C9>(K), (double)kc<KC_AT_C7>(K));
    p = __builtin_fma(s, p, (double)kc<KC_AT_C5>(K));
    p = __builtin_fma(s, p, (double)kc<KC_AT_C3>(K));
    double a = (double)tab[i] + __builtin_fma(r * s, p, r);
    a = ay > ax ? kc<KC_HALF_PI>(K) - a : a;
    if constexpr (!XPOS) {
        a = x < 0 ? kc<KC_PI>(K) - a : a;
        a = mx > 0 ? a : 0.0;
    }
    return __builtin_copysign(a, y);
}
// single-precision atan2 for the fp32 stepper: t = min/max through v_rcp_f32, atan t = t P(t^2) with a degree-7 near-minimax P
// (coefficients as VOP2 literals: one instruction per term); 25 instructions against the library's ~55. Absolute error: the polynomial
// 1.09e-7, with v_rcp_f32 and the roundings <= 3.0e-7 in the first octant, <= 4.1e-7 after π/2 - a (XPOS), <= 6.1e-7 after π - a, where
// one ulp of the result is 2.4e-7 (the count: tests/math_cases.py, ATAN2_FAST_BOUND; "2e-7 absolute" stood here: the host measures
// 3.5e-7 near ±π with a correctly rounded reciprocal). DOMAIN and NaN as atan2_tab: max(|x|, |y|) in [1e-30, 1e30] or both zero.
template <bool XPOS = false>
FBD float atan2_fast(float y, float x) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const float mx = __builtin_fmaxf(ax, ay), mn = __builtin_fminf(ax, ay);
    const float t = mn * __builtin_amdgcn_rcpf(mx), s = t * t;
    float p = -0.00478042708709836f;
    p = __builtin_fmaf(p, s, 0.024557026103138924f); p = __builtin_fmaf(p, s, -0.05990458279848099f);
    p = __builtin_fmaf(p, s, 0.09942749887704849f); p = __builtin_fmaf(p, s, -0.1402941644191742f);
    p = __builtin_fmaf(p, s, 0.19971375167369843f); p = __builtin_fmaf(p, s, -0.3333209455013275f);
    p = __builtin_fmaf(p, s, 0.9999999403953552f);
    float a = t * p;
    a = ay > ax ? 1.5707963267948966f - a : a;
    if constexpr (!XPOS) {
        a = x < 0 ? 3.141592653589793f - a : a;
        a = mx > 0 ? a : 0.0f;   // atan2(0, 0) = 0 (0 * rcp(0) is NaN)
    }
    return __builtin_copysignf(a, y);
}
// exp / log of the stepping kernels' fast path. fp64: the library's; fp32: v_exp_f32 / v_log_f32 on the base-2 forms (1 ulp of
// the hardware functions, 3 instructions instead of ~15: the fp32 stepper is VALU-issue-bound, every instruction counts). Absolute error
// on the ISA's arguments, from that 1 ulp, the fp32 constant and the product's rounding: exp_step <= 2.6e-7 on [-2, 0.2], log_step
// <= 5.8e-8 on [0.69, 1.03] (tests/math_cases.py, EXP_STEP_BOUND / LOG_STEP_BOUND).
FBD real exp_step(real x) {
    if constexpr (sizeof(real) == 8) return exp(x); else return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
}
FBD real log_step(real x) {
    if constexpr (sizeof(real) == 8) return log(x); else return __builtin_amdgcn_logf(x) * 0.6931471805599453f;
}
template <bool XPOS = false, class KP = KLit>
FBD real atan2_step(real y, real x, lds_cptr tab, const KP& K = KP{}) {   // the stepping kernels' atan2, by arithmetic type
    if constexpr (sizeof(real) == 8) return atan2_tab<XPOS>(y, x, tab, K); else return atan2_fast<XPOS>(y, x);
}
// log u for u near 1 (the troposphere's temperature ratio, 0.7 .. 1.1): 2 atanh w, w = (u - 1)/(u + 1), |w| < 0.18, ten series
// terms; 45 instructions against the library's 98. Error 1.93 ulp on the host, <= 2.43 with the device's 1-ulp division ("<= 1.5" stood
// here). DOMAIN [0.65, 1.5] (12 ulp off at 0.6 already); the one caller stays within [0.6997, 1.03]: h0 <= 11 km, T_sl saturated to
// 288.15 +- 50 K by the host, h >= H_MIN (tests/test_math_primitives_host.py pins that range).
FB_KC(KC_LN_C3, 2.0 / 3); FB_KC(KC_LN_C5, 2.0 / 5); FB_KC(KC_LN_C7, 2.0 / 7); FB_KC(KC_LN_C9, 2.0 / 9); FB_KC(KC_LN_C11, 2.0 / 11);
FB_KC(KC_LN_C13, 2.0 / 13); FB_KC(KC_LN_C15, 2.0 / 15); FB_KC(KC_LN_C17, 2.0 / 17); FB_KC(KC_LN_C19, 2.0 / 19); FB_KC(KC_LN_C21, 2.0 / 21);
template <class KP = KLit>
FBD double log_near1(double u, const KP& K = KP{}) {
    const double w = (u - 1) / (u + 1), s = w * w;
    double p = kc<KC_LN_C21>(K);
    p = __builtin_fma(s, p, (double)kc<KC_LN_C19>(K)); p = __builtin_fma(s, p, (double)kc<KC_LN_C17>(K)); p = __builtin_fma(s, p, (double)kc<KC_LN_C15>(K));
    p = __builtin_fma(s, p, (double)kc<KC_LN_C13>(K)); p = __builtin_fma(s, p, (double)kc<KC_LN_C11>(K)); p = __builtin_fma(s, p, (double)kc<KC_LN_C9>(K));
    p = __builtin_fma(s, p, (double)kc<KC_LN_C7>(K)); p = __builtin_fma(s, p, (double)kc<KC_LN_C5>(K)); p = __builtin_fma(s, p, (double)kc<KC_LN_C3>(K));
    return __builtin_fma(w * s, p, w + w);
}

// sin and cos together for the stepping kernels' NED mechanisation (its states are angles: six library sincos, two tan and two cos per
// evaluation, ~1 200 instructions, made NED 35 % slower than ECEF): k = round(x 2/pi), r = x - k pi/2 by a three-constant
// Cody-Waite reduction carried by fma (exact to 1e-17 for |k| < 2^20), Taylor polynomials of sin r / cos r on |r| <= pi/4 to r^17 / r^16
// (truncation < 1e-17), quadrant by k mod 4. ~40 instructions, <= 1.5 ulp for |x| < 1e6 rad (a heading state that winds up through
// 160 000 full turns; measured 1.48 ulp on the host), degrading by one ulp per further factor of two; NaN and inf give NaN like the library.
FBD void sincos_step(double x, double& s, double& c) {
    const double k = __builtin_rint(x * 0.6366197723675814);
    double r = __builtin_fma(-k, 1.5707963267948966, x);
    r = __builtin_fma(-k, 6.123233995736766e-17, r);
    r = __builtin_fma(-k, -1.4973849048591698e-33, r);
    const double z = r * r;
    double ps = 1.0 / 355687428096000.0, pc = 1.0 / 20922789888000.0;
    ps = __builtin_fma(z, ps, -1.0 / 1307674368000.0); pc = __builtin_fma(z, pc, -1.0 / 87178291200.0);
    ps = __builtin_fma(z, ps, 1.0 / 6227020800.0);     pc = __builtin_fma(z, pc, 1.0 / 479001600.0);
    ps = __builtin_fma(z, ps, -1.0 / 39916800.0);      pc = __builtin_fma(z, pc, -1.0 / 3628800.0);
    ps = __builtin_fma(z, ps, 1.0 / 362880.0);         pc = __builtin_fma(z, pc, 1.0 / 40320.0);
    ps = __builtin_fma(z, ps, -1.0 / 5040.0);          pc = __builtin_fma(z, pc, -1.0 / 720.0);
    ps = __builtin_fma(z, ps, 1.0 / 120.0);            pc = __builtin_fma(z, pc, 1.0 / 24.0);
    ps = __builtin_fma(z, ps, -1.0 / 6.0);             pc = __builtin_fma(z, pc, -0.5);
    const double sr = __builtin_fma(r * z, ps, r), cr = __builtin_fma(z, pc, 1.0);
    const int q = (int)k & 3;
    const double s0 = (q & 1) ? cr : sr, c0 = (q & 1) ? sr : cr;
    s = (q & 2) ? -s0 : s0;
    c = ((q + 1) & 2) ? -c0 : c0;
}
FBD void sincos_step(float x, float& s, float& c) { ::sincosf(x, &s, &c); }

// EGM96 geoid height at a location given by its n-vector (geodesy.jl:103-106, 186-211).
// Bilinear on the uniform grid lat ∈ [-π/2, π/2] (721), lon ∈ [0, 2π] (1441), linear extrapolation.
// the EGM96 cell a point fell into: grid indices, fractional grid coordinates and the four samples
struct GeoidCell { int i, j; real xi, xj, a00, a10, a01, a11; };
template <bool FAST = false, class KP = KLit>
FBD real geoid_height(const Tables& T, v3 n, real& lat, real& lon, GeoidCell& gc, const KP& K = KP{}) {
    if constexpr (FAST) {
        lat = atan2_step<true>(n.z, sqrt(n.x * n.x + n.y * n.y, K), T.rk + LDS_ATAN, K);   // (|n| ~ 1: never both zero)
        lon = atan2_step(n.y, n.x, T.rk + LDS_ATAN, K);
    } else {
        lat = atan2(n.z, sqrt(n.x * n.x + n.y * n.y));
        lon = atan2(n.y, n.x);
    }
    // λ = mod(lon + 2π, 2π) (geodesy.jl:209) without calling fmod: lon ∈ [-π, π], so t = fl(lon + 2π) ∈ [π, 3π] and the
    // remainder is t itself or t - 2π, which is exact (Sterbenz). Branch-free on purpose: library fmod brings divergent
    // control flow into the stepping kernel, and with it the spill-placement bug tools/check_isa_spills.py guards against.
    const real t2 = lon + kc<KC_TWO_PI>(K);
    const real lam = t2 >= kc<KC_TWO_PI>(K) ? t2 - kc<KC_TWO_PI>(K) : t2;
    const real xi = (lat + kc<KC_HALF_PI>(K)) * kc<KC_GEOID_PER_RAD>(K);
    const real xj = lam * kc<KC_GEOID_PER_RAD>(K);
    const int i = min(max((int)floor(xi), 0), 719);
    const int j = min(max((int)floor(xj), 0), 1439);
    const real wi = xi - i, wj = xj - j;
    const float* p = T.egm96 + i + 721 * j;
    const real a00 = p[0], a10 = p[1], a01 = p[721], a11 = p[722];
    gc = {i, j, xi, xj, a00, a10, a01, a11};
    return (1 - wi) * ((1 - wj) * a00 + wj * a01) + wi * ((1 - wj) * a10 + wj * a11);
}
template <bool FAST = false, class KP = KLit>
FBD real geoid_height(const Tables& T, v3 n, real& lat, real& lon, const KP& K = KP{}) {
    GeoidCell gc;
    return geoid_height<FAST>(T, n, lat, lon, gc, K);
}
FBD real geoid_height(const Tables& T, v3 n) {
    real la, lo;
    return geoid_height(T, n, la, lo);
}
// Geoid height of a point (dlat, dlon) [rad] away from the one whose cell is gc — a wheel, a couple of metres from the body
// origin: the same bilinear interpolant on the same samples, without a second pair of atan2 and (almost always) without a second
// gather; a point that has crossed into a neighbouring cell fetches that cell's samples.
FBD real geoid_height_near(const Tables& T, const GeoidCell& gc, real dlat, real dlon) {
    const real xi = gc.xi + dlat * (720 / PI);
    real xj = gc.xj + dlon * (1440 / (2 * PI));
    xj = xj >= 1440 ? xj - 1440 : (xj < 0 ? xj + 1440 : xj);   // (the longitude seam)
    const int i = min(max((int)floor(xi), 0), 719);
    const int j = min(max((int)floor(xj), 0), 1439);
    const real wi = xi - i, wj = xj - j;
    real a00 = gc.a00, a10 = gc.a10, a01 = gc.a01, a11 = gc.a11;
    if (i != gc.i || j != gc.j) {
        const float* p = T.egm96 + i + 721 * j;
        a00 = p[0]; a10 = p[1]; a01 = p[721]; a11 = p[722];
    }
    return (1 - wi) * ((1 - wj) * a00 + wj * a01) + wi * ((1 - wj) * a10 + wj * a11);
}

// ECEF -> (n-vector, ellipsoidal altitude): Fukushima, one Halley step (geodesy.jl:367-412)
FBD void geodetic_from_ecef(v3 r, v3& n, real& h) {
    using namespace wgs;
    // fp32 instance: the intermediate terms grow like a0^7 (1e47 in metres) and overflow, so it works in Earth radii
    constexpr bool SCALED = sizeof(real) == 4;
    constexpr real A = SCALED ? FBL(1.0) : a;
    if (SCALED) r = (1 / a) * r;
    const real p2 = r.x * r.x + r.y * r.y;
    const real p = sqrt(p2);
    const real az = fabs(r.z);
    constexpr real c = A * e2;
    constexpr real ec2 = 1 - e2;
    const real ec = sqrt(ec2);
    const real zc = ec * az;
    const real s0 = az;
    const real c0 = ec * p;
    const real a0 = sqrt(s0 * s0 + c0 * c0);
    const real a03 = a0 * a0 * a0;
    const real b0 = FBL(1.5) * c * s0 * c0 * ((p * s0 - zc * c0) * a0 - c * s0 * c0);
    const real s1 = (zc * a03 + c * (s0 * s0 * s0)) * a03 - b0 * s0;
    const real c1 = (p * a03 - c * (c0 * c0 * c0)) * a03 - b0 * c0;
    const real cc = ec * c1;
    const real s12 = s1 * s1, cc2 = cc * cc;
    h = (p * cc + s0 * s1 - A * sqrt(ec2 * s12 + cc2)) / sqrt(s12 + cc2);
    if (SCALED) h = h * a;
    const real sgn = (r.z > 0) ? FBL(1.0) : ((r.z < 0) ? -FBL(1.0) : FBL(0.0));
    real cos_phi, sin_phi;
    if (s1 < cc) {
        const real t = s1 / cc;
        cos_phi = 1 / sqrt(1 + t * t);
        sin_phi = t * cos_phi * sgn;
    } else {
        const real t = cc / s1;
        const real as = 1 / sqrt(1 + t * t);
        cos_phi = t * as;
        sin_phi = as * sgn;
    }
    const real cl = p > 0 ? r.x / p : FBL(1.0);
    const real sl = p > 0 ? r.y / p : FBL(0.0);
    v3 u = {cos_phi * cl, cos_phi * sl, sin_phi};
    const real inv = 1 / norm(u);  // NVector constructor normalises (geodesy.jl:47-51)
    n = inv * u;
}
// Somigliana gravity with altitude correction (geodesy.jl:451-467)
FBD real normal_gravity(real nz, real h) {
    using namespace wgs;
    const real s2 = nz * nz;
    const real g0 = g_a * (1 + k_g * s2) * rsqrt(1 - e2 * s2);
    return g0 * (1 - 2 / a * (1 + f + m - 2 * f * s2) * h + 3 / a2 * (h * h));
}

// ltf(n_e) = Rz(λ) ∘ Ry(-(ϕ + π/2)) with ψ_nw = 0 (geodesy.jl:132-135), λ = atan2(n_y, n_x), -(ϕ + π/2) = atan2(-p, -n_z),
// p = |(n_x, n_y)|: built from half-angle cos/sin pairs, no atan2 / sincos
FBD quat ltf_quat(v3 n) {
    real sl, cl, sp, cp;
    half_angle_cs(n.y, n.x, cl, sl);
    half_angle_cs(-sqrt(n.x * n.x + n.y * n.y), -n.z, cp, sp);
    return {cl * cp, -(sl * sp), cl * sp, sl * cp};
}

// ---------------------------------------------------------------------------------------------
// table lookups (Interpolations.jl semantics: Gridded(Linear) knot search = searchsortedlast clamped)
struct loc { int i; real w; };
// k: knots in LDS; rk: reciprocal spacings 1/(k[j+1]-k[j]) in LDS (computed once per workgroup), so the
// interpolation weight costs a multiply instead of an fp64 division (~12 VALU instructions each, ~20 per RHS).
// SLOT >= 0: the table has a contiguous copy of its first, last and every S-th knot behind the blob (tables.h: LDS_AUX), gb = the blob
template <int N, bool SCALAR = false, int SLOT = -1>
FBD loc grid_locate(lds_cptr k, lds_cptr rk, real x, bool flat_lo, bool flat_hi, gk_cptr g = nullptr, gk_cptr gb = nullptr) {
    if constexpr (SCALAR && N > SCALAR_KNOTS_MIN) {   // (short tables stay in LDS: no scalar-load round trip)
        constexpr bool TWO_LEVEL = N >= 11;   // coarse-then-fine knot scan
        if constexpr (TWO_LEVEL && SLOT >= 0) {   // one scalar load brings the clamps and the coarse knots
            static_assert(2 + (N - 2) / (N >= 20 ? 4 : 3) <= AUX_STRIDE, "coarse knots must fit their slot");
            constexpr int S = N >= 20 ? 4 : 3, G = (N - 2) / S;
            gk_cptr gc = gb + LDS_AUX + AUX_STRIDE * SLOT;
            if (flat_lo) x = fmax(x, (real)gc[0]);
            if (flat_hi) x = fmin(x, (real)gc[1]);
            int c = 0;
#pragma unroll
            for (int m = 1; m <= G; m++) c += ((real)gc[1 + m] <= x) ? 1 : 0;
            lds_cptr kf = k + S * c;
            int i = S * c;
#pragma unroll
            for (int r = 1; r < S; r++) i += (kf[r] <= x) ? 1 : 0;
            i = min(i, N - 2);
            return {i, (x - k[i]) * rk[i]};
        }
        if (flat_lo) x = fmax(x, (real)g[0]);       // (one v_max / v_min each; a compare-and-select pair costs four issue slots in fp64)
        if (flat_hi) x = fmin(x, (real)g[N - 1]);
        int i = 0;
        if constexpr (TWO_LEVEL) {
            // Every S-th interior knot from SGPRs, then the S - 1 knots above the coarse position from LDS: (N-2)/S + S - 1 compares
            // instead of N - 2 (a compare-and-count is 2-3 issue slots per knot): -170 instructions per RHS, +6 % on the fp64 stepper.
            // The fine reads of the top group may run past the last interior knot (into the table's last knot and the values
            // behind it): the final min() discards whatever they counted.
            constexpr int S = N >= 20 ? 4 : 3, G = (N - 2) / S;
            int c = 0;
#pragma unroll
            for (int m = 1; m <= G; m++) c += ((real)g[S * m] <= x) ? 1 : 0;
            lds_cptr kf = k + S * c;
            i = S * c;
#pragma unroll
            for (int r = 1; r < S; r++) i += (kf[r] <= x) ? 1 : 0;
            i = min(i, N - 2);
        } else {
#pragma unroll
            for (int j = 1; j <= N - 2; j++) i += ((real)g[j] <= x) ? 1 : 0;   // (hand-scheduled v_cmp_e64 / v_addc triples were tried: no gain)
        }
        return {i, (x - k[i]) * rk[i]};   // the knot below x and its reciprocal spacing are lane-dependent: LDS
    }
    if (flat_lo) x = fmax(x, k[0]);
    if (flat_hi) x = fmin(x, k[N - 1]);
    int i = 0;
#pragma unroll
    for (int j = 1; j <= N - 2; j++) i += (k[j] <= x) ? 1 : 0;  // knots ascending: count = index of last knot <= x
    return {i, (x - k[i]) * rk[i]};
}
// uniform knots a + j (b-a)/(n-1): a, b, n are literals at every call site, so the reciprocal step folds at compile time
// (rstep: the reciprocal step (n - 1) / (b - a), for a caller that keeps it — and a, b — in registers: "resident-capable constants")
FBD loc range_locate(real a, real b, real rstep, int n, real x, bool flat) {
    if (flat) x = fmin(fmax(x, a), b);
    const real xi = (x - a) * rstep;
    const int i = min(max((int)floor(xi), 0), n - 2);
    return {i, xi - i};
}
FBD loc range_locate(real a, real b, int n, real x, bool flat) { return range_locate(a, b, (n - 1) / (b - a), n, x, flat); }
// Table values are read one ds_read_b64 each: left to itself the compiler pairs neighbouring elements into ds_read2_b64, and for
// ONE wave per SIMD reading lane-dependent (scattered, bank-conflicting) addresses a ds_read2_b64 costs the wave 24-43 issue cycles
// against 2 x 6-8 for two single reads (tools/microbench/lds.hip: bilinear corners as 2 x read2 +87 cycles, as 4 x read +25).
// So the reads go through a volatile pointer, which the load/store optimizer leaves alone.
FBD real tab(lds_cptr v, int i) {
    // (fp64 only: the fp32 stepper runs two waves per SIMD, where a ds_read2_b32 is the cheaper form — measured 6.72e9 vs 6.46e9)
    if constexpr (sizeof(real) == 8) return *(volatile __attribute__((address_space(3))) const real*)(v + i);
    return v[i];
}
FBD real lerp1(lds_cptr v, loc l) { return (1 - l.w) * tab(v, l.i) + l.w * tab(v, l.i + 1); }
FBD real lerp2(lds_cptr v, int n1, loc l1, loc l2) {
    lds_cptr p = v + l1.i + n1 * l2.i;
    const real p00 = tab(p, 0), p10 = tab(p, 1), p01 = tab(p, n1), p11 = tab(p, n1 + 1);
    return (1 - l1.w) * ((1 - l2.w) * p00 + l2.w * p01) + l1.w * ((1 - l2.w) * p10 + l2.w * p11);
}

// ---------------------------------------------------------------------------------------------
// Atmosphere (FlightPhysics/src/atmosphere.jl:22-34, 99-135)
namespace isa {
constexpr real R = FBL(287.05287), gamma = FBL(1.40), beta_s = FBL(1.458e-6), S = FBL(110.4);
constexpr real T_std = FBL(288.15), p_std = FBL(101325.0), rho_std = p_std / (R * T_std), g_std = FBL(9.80665);
}  // namespace isa
constexpr real isa_sqrt_T_std = FBL(16.97498159056439);   // sqrt(288.15)
// lnp = log(p / p_sl), the sum of the layers' exponents (the engine model wants log(p / p_std) again, piston.jl:38-41).
// The troposphere is evaluated straight-line for every lane (same arithmetic as the layer loop's first pass); the loop over
// the higher layers is only entered above 11 km.
FB_KC(KC_ISA_H11, 11000); FB_KC(KC_ISA_BETA0, -FBL(6.5e-3));
FB_KC(KC_ISA_LNP, -isa::g_std / (-FBL(6.5e-3) * isa::R));            // the exponent of the troposphere's pressure law, 5.2559
FB_KC(KC_ISA_CFRAC, -isa::g_std / (-FBL(6.5e-3) * isa::R) - 5);      // ... and what is left of it behind u0^5
FB_KC(KC_EXP_C3, FBL(1.0) / 6); FB_KC(KC_EXP_C4, FBL(1.0) / 24); FB_KC(KC_EXP_C5, FBL(1.0) / 120); FB_KC(KC_EXP_C6, FBL(1.0) / 720);
FB_KC(KC_EXP_C7, FBL(1.0) / 5040); FB_KC(KC_EXP_C8, FBL(1.0) / 40320); FB_KC(KC_EXP_C9, FBL(1.0) / 362880);
template <bool FAST = false, class KP = KLit>
FBD void isa_data(real h, real T_sl, real p_sl, real& T, real& p, real& lnp, int32_t& st, const KP& K = KP{}) {
    constexpr real beta[7] = {-FBL(6.5e-3), 0, FBL(1e-3), FBL(2.8e-3), 0, -FBL(2.8e-3), -FBL(2e-3)};
    constexpr real hc[7] = {11000, 20000, 32000, 47000, 51000, 71000, 84852};
    static_assert(KC<KC_ISA_H11>::v == hc[0] && KC<KC_ISA_BETA0>::v == beta[0] && KC<KC_ISA_LNP>::v == -isa::g_std / (beta[0] * isa::R), "the first layer's constants");
    const real h0 = fmin(h, kc<KC_ISA_H11>(K));
    T = T_sl + kc<KC_ISA_BETA0>(K) * h0;
    const real u0 = 1 + kc<KC_ISA_BETA0>(K) / T_sl * h0;
    real ln_u0;
    if constexpr (FAST && sizeof(real) == 8) ln_u0 = log_near1(u0, K); else if constexpr (FAST) ln_u0 = log_step(u0); else ln_u0 = log(u0);
    lnp = kc<KC_ISA_LNP>(K) * ln_u0;
    if constexpr (FAST && sizeof(real) == 8) {
        // p / p_sl = u0^c, c = g / (beta R) = 5.2559: u0^5 by multiplication, u0^(c - 5) = exp(y) with |y| = 0.256 |ln u0| < 0.1 straight from
        // the series (no range reduction, degree 9: the truncation is 2.8e-17 at |y| = 0.1, measured by tests/test_math_primitives_host.py) — 15 arithmetic instructions instead of the library exp's ~40
        constexpr real cfrac = KC<KC_ISA_CFRAC>::v;
        static_assert(cfrac == -isa::g_std / (beta[0] * isa::R) - 5 && cfrac > FBL(0.25) && cfrac < FBL(0.26), "the exponent of the troposphere's pressure law");
        const real y = kc<KC_ISA_CFRAC>(K) * ln_u0;
        real e = kc<KC_EXP_C9>(K);
        e = __builtin_fma(e, y, kc<KC_EXP_C8>(K)); e = __builtin_fma(e, y, kc<KC_EXP_C7>(K)); e = __builtin_fma(e, y, kc<KC_EXP_C6>(K));
        e = __builtin_fma(e, y, kc<KC_EXP_C5>(K)); e = __builtin_fma(e, y, kc<KC_EXP_C4>(K)); e = __builtin_fma(e, y, kc<KC_EXP_C3>(K));
        e = __builtin_fma(e, y, FBL(0.5)); e = __builtin_fma(e, y, FBL(1.0)); e = __builtin_fma(e, y, FBL(1.0));
        const real u2 = u0 * u0, u4 = u2 * u2;
        p = (p_sl * (u4 * u0)) * e;
    } else if constexpr (FAST) p = p_sl * exp_step(lnp); else p = p_sl * exp(lnp);
    if (h < kc<KC_ISA_H11>(K)) return;
    real hb = hc[0], Tb = T, pb = p;
    bool done = false;
#pragma unroll 1
    for (int i = 1; i < 7 && !done; i++) {
        const real hh = (h < hc[i]) ? h : hc[i];
        done = h < hc[i];
        const real Tn = Tb + beta[i] * (hh - hb);
        real e;
        if (beta[i] != FBL(0.0)) e = -isa::g_std / (beta[i] * isa::R) * log(1 + beta[i] / Tb * (hh - hb));
        else e = -isa::g_std / (isa::R * Tb) * (hh - hb);
        const real pn = pb * exp(e);
        lnp += e;
        T = Tn; p = pn;
        hb = hc[i]; Tb = Tn; pb = pn;
    }
    if (!done) st |= FB_ST_ISA_RANGE;
}

// ---------------------------------------------------------------------------------------------
// continuous PI compensator with anti-windup (FlightPhysics/src/control.jl:52-81), one channel
FBD real pi_ode(real k_p, real k_i, real k_l, real lo, real hi, real input, real x_i, real& output) {
    const real out_free = k_p * input + x_i;
    output = fmin(fmax(out_free, lo), hi);
    const int sat = (out_free >= hi ? 1 : 0) - (out_free <= lo ? 1 : 0);
    const bool halted = (input * sat) > 0;  // sat_ext is never driven on this path (stays 0)
    return (halted ? FBL(0.0) : k_i * input) - k_l * x_i;
}

// ---------------------------------------------------------------------------------------------
// Model constants of Cessna172Sv0
namespace c172 {
constexpr real D2R = PI / 180;
// aero (FlightApps/src/c172/c172.jl:247-258)
constexpr real S = FBL(16.165), b = FBL(10.912), c = FBL(1.494), V_min = FBL(1.0), tau_filt = FBL(0.02);
constexpr real de_lo = -28 * D2R, de_hi = 23 * D2R, da_lo = -20 * D2R, da_hi = 20 * D2R;
constexpr real dr_lo = -16 * D2R, dr_hi = 16 * D2R, df_lo = FBL(0.0), df_hi = 30 * D2R;
constexpr real alpha_stall_lo = FBL(0.09), alpha_stall_hi = FBL(0.36);
// landing gear (c172.jl:442-476): strut attachment points, dampers (k_s, k_d_ext, k_d_cmp)
constexpr real ldg_r[3][3] = {{-FBL(0.381), -FBL(1.092), FBL(1.902)}, {-FBL(0.381), FBL(1.092), FBL(1.902)}, {FBL(1.27), FBL(0.0), FBL(1.9)}};
constexpr real ldg_ks[3] = {39404, 39404, 26269};
constexpr real ldg_kd[3] = {9340, 9340, 3503};
constexpr real psi_max = PI / 6;  // DirectSteering default (FlightPhysics/src/landinggear.jl:47-49)
// contact friction regulator (landinggear.jl:401-409)
constexpr real frc_kp = FBL(5.0), frc_ki = FBL(400.0), frc_kl = FBL(0.2);
// power plant (FlightApps/src/c172/c172s/c172s.jl:16-34; FlightPhysics/src/piston.jl:25-35)
constexpr real P_rated = FBL(735.49875) * 200, w_rated = 2700 * PI / 30, w_stall = 300 * PI / 30, w_idle = 600 * PI / 30;
constexpr real tau_start = 40, J_eng = FBL(0.05);
constexpr real f_lean = FBL(0.0625), f_rich = FBL(0.0950);
constexpr real prop_d = FBL(2.0), prop_Jxx = FBL(0.3), prop_r[3] = {FBL(2.055), FBL(0.0), FBL(0.833)};
// airframe mass (c172.jl:26-35): RigidBodyDistribution(767, diag(820,1164,1702)) at r = (0.056, 0, 0.582)
constexpr real afm_m = FBL(767.0), afm_J[3] = {FBL(820.0), FBL(1164.0), FBL(1702.0)}, afm_r[3] = {FBL(0.056), FBL(0.0), FBL(0.582)};
// payload slots (c172.jl:513-519) and fuel tanks (c172.jl:628-629)
constexpr real pld_r[5][3] = {{FBL(0.183), -FBL(0.356), FBL(0.899)}, {FBL(0.183), FBL(0.356), FBL(0.899)}, {-FBL(0.681), -FBL(0.356), FBL(0.899)}, {-FBL(0.681), FBL(0.356), FBL(0.899)}, {-FBL(1.316), FBL(0.0), FBL(0.899)}};
constexpr real fuel_r[2][3] = {{FBL(0.325), -FBL(2.845), FBL(0.0)}, {FBL(0.325), FBL(2.845), FBL(0.0)}};
constexpr real m_full = FBL(114.4), m_res = FBL(1.0);
}  // namespace c172

FBD real clampd(real v, real lo, real hi) { return fmin(fmax(v, lo), hi); }
struct Env {  // fb_params subset, wave-uniform (SGPRs)
    real T_sl, p_sl, wind_n, wind_e, wind_d, h_trn;
    int surface;
    real ln_p_sl;   // log(p_sl / p_std), filled by the host
    real k_rt;      // (p_sl / p_std)^(beta R / 2 g) / sqrt(T_sl), filled by the host (see the engine block of rhs)
};
// Per-aircraft inputs, constant during a launch. Only what the airborne path needs every RHS lives in
// registers (deflections are pre-scaled once); the ground-only inputs (steering, brakes) are fetched from
// global memory inside the rare contact branch.
struct Inputs {
    static constexpr bool pld_precomputed = false; static constexpr bool aero_precomputed = false;
    real de, da, dr, df;     // surface deflections [rad] (c172s.jl:92-120 sign conventions + c172.jl:337-340 scaling)
    real throttle, mixture;  // engine (Ranged [0,1])
    real m_pld[5];           // payload masses (Ranged [0,100])
    int ui;                    // FB_UI_* bits
    const double* u_glob;      // &u[0*n + i] for ground-only inputs; may be null (then they read as 0)
    int64_t n;
    FBD real get_de() const { return de; }
    FBD real get_da() const { return da; }
    FBD real get_dr() const { return dr; }
    FBD real get_df() const { return df; }
    FBD real get_throttle() const { return throttle; }
    FBD real get_mixture() const { return mixture; }
    FBD real get_m_pld(int k) const { return m_pld[k]; }
    FBD real get_steering() const {
        return u_glob ? clampd(clampd(u_glob[FB_U_RUDDER * n], -1, 1) + clampd(u_glob[FB_U_RUDDER_OFFSET * n], -1, 1), -1, 1) : FBL(0.0);
    }
    FBD real get_brake(int g) const { return u_glob ? clampd(u_glob[(g == 0 ? FB_U_BRAKE_LEFT : FB_U_BRAKE_RIGHT) * n], 0, 1) : FBL(0.0); }
};
// The same eleven values parked in an LDS panel [11][STRIDE] (row = quantity, column = lane) and read at the
// point of use: the stepping kernel cannot afford 22 VGPRs for values that are touched once per RHS.
template <int STRIDE>
struct InputsLds {
    static constexpr bool pld_precomputed = false; static constexpr bool aero_precomputed = false;
    lds_cptr p;                // &panel[lane]
    int ui;
    const double* u_glob;
    int64_t n;
    FBD real get_de() const { return p[0 * STRIDE]; }
    FBD real get_da() const { return p[1 * STRIDE]; }
    FBD real get_dr() const { return p[2 * STRIDE]; }
    FBD real get_df() const { return p[3 * STRIDE]; }
    FBD real get_throttle() const { return p[4 * STRIDE]; }
    FBD real get_mixture() const { return p[5 * STRIDE]; }
    FBD real get_m_pld(int k) const { return p[(6 + k) * STRIDE]; }
    FBD real get_steering() const {
        return u_glob ? clampd(clampd(u_glob[FB_U_RUDDER * n], -1, 1) + clampd(u_glob[FB_U_RUDDER_OFFSET * n], -1, 1), -1, 1) : FBL(0.0);
    }
    FBD real get_brake(int g) const { return u_glob ? clampd(u_glob[(g == 0 ? FB_U_BRAKE_LEFT : FB_U_BRAKE_RIGHT) * n], 0, 1) : FBL(0.0); }
    FBD void store(lds_ptr q, const Inputs& in) {
        q[0 * STRIDE] = in.de; q[1 * STRIDE] = in.da; q[2 * STRIDE] = in.dr; q[3 * STRIDE] = in.df;
        q[4 * STRIDE] = in.throttle; q[5 * STRIDE] = in.mixture;
#pragma unroll
        for (int k = 0; k < 5; k++) q[(6 + k) * STRIDE] = in.m_pld[k];
        p = q; ui = in.ui; u_glob = in.u_glob; n = in.n;
    }
};
constexpr int INPUT_PANEL_ROWS = 11;
// Cessna172X (fly-by-wire): surfaces, throttle, nose-wheel steering and brakes follow the actuator POSITIONS, which are
// states (device rows 27..33: throttle, aileron, elevator, rudder, flaps, brake_left, brake_right), saturated to their
// Ranged type on the way out (Actuator1.f_ode!: pos = R(x.p), c172x.jl:45; assign!, c172x.jl:127-143: aero.u.e = -elevator.pos,
// aero.u.a = aileron.pos, aero.u.r = -rudder.pos, aero.u.f = flaps.pos, throttle, steering = rudder.pos, brakes).
// Mixture and payload are launch constants read from global memory at the point of use (L1/L2 resident).
constexpr int X2_ACT = FB_NX;  // device row of the first actuator position
struct InputsX {
    static constexpr bool pld_precomputed = false; static constexpr bool aero_precomputed = false;
    const real* xa;      // the seven actuator positions of the state being evaluated (caller's registers)
    const double* u_glob;  // &u[0 * n + i]
    int64_t n;
    int ui;
    FBD real pos(int k) const { return clampd(xa[k], (k == FB_ACT_THROTTLE || k >= FB_ACT_FLAPS) ? FBL(0.0) : -FBL(1.0), FBL(1.0)); }
    FBD real get_de() const { return c172::de_lo + (c172::de_hi - c172::de_lo) / 2 * (clampd(-pos(FB_ACT_ELEVATOR), -1, 1) + 1); }
    FBD real get_da() const { return c172::da_lo + (c172::da_hi - c172::da_lo) / 2 * (clampd(pos(FB_ACT_AILERON), -1, 1) + 1); }
    FBD real get_dr() const { return c172::dr_lo + (c172::dr_hi - c172::dr_lo) / 2 * (clampd(-pos(FB_ACT_RUDDER), -1, 1) + 1); }
    FBD real get_df() const { return c172::df_lo + (c172::df_hi - c172::df_lo) / 1 * (clampd(pos(FB_ACT_FLAPS), 0, 1) - 0); }
    FBD real get_throttle() const { return pos(FB_ACT_THROTTLE); }
    FBD real get_mixture() const { return clampd(u_glob[FB_U_MIXTURE * n], 0, 1); }
    FBD real get_m_pld(int k) const { return clampd(u_glob[(FB_U_M_PILOT + k) * n], 0, 100); }
    FBD real get_steering() const { return pos(FB_ACT_RUDDER); }
    FBD real get_brake(int g) const { return pos(g == 0 ? FB_ACT_BRAKE_LEFT : FB_ACT_BRAKE_RIGHT); }
};
constexpr real ACT_TAU = FBL(1.0) / 20;  // Actuator1 time constant, c172x.jl:21
// InputsX with the payload's mass-property sums taken once per launch (see InputsAgg below)
struct InputsXAgg : InputsX {
    static constexpr bool pld_precomputed = true;
    real pld_M, pld_J[6];
    real pld_Mr[3];
    FBD real get_pld_M() const { return pld_M; }
    FBD real get_pld_Mr(int k) const { return pld_Mr[k]; }
    FBD real get_pld_J(int k) const { return pld_J[k]; }
};
// mechanical actuation + Ranged saturation + linear_scaling, from the raw FB_U_* inputs
FBD void make_inputs(Inputs& in, const double* u, int64_t stride, int ui) {
    using namespace c172;
    const real ail = clampd(u[FB_U_AILERON * stride], -1, 1) + clampd(u[FB_U_AILERON_OFFSET * stride], -1, 1);
    const real elv = clampd(u[FB_U_ELEVATOR * stride], -1, 1) + clampd(u[FB_U_ELEVATOR_OFFSET * stride], -1, 1);
    const real rud = clampd(u[FB_U_RUDDER * stride], -1, 1) + clampd(u[FB_U_RUDDER_OFFSET * stride], -1, 1);
    const real aero_e = clampd(-elv, -1, 1), aero_a = clampd(ail, -1, 1), aero_r = clampd(-rud, -1, 1);
    const real aero_f = clampd(u[FB_U_FLAPS * stride], 0, 1);
    in.de = de_lo + (de_hi - de_lo) / 2 * (aero_e + 1);
    in.da = da_lo + (da_hi - da_lo) / 2 * (aero_a + 1);
    in.dr = dr_lo + (dr_hi - dr_lo) / 2 * (aero_r + 1);
    in.df = df_lo + (df_hi - df_lo) / 1 * (aero_f - 0);
    in.throttle = clampd(u[FB_U_THROTTLE * stride], 0, 1);
    in.mixture = clampd(u[FB_U_MIXTURE * stride], 0, 1);
#pragma unroll
    for (int k = 0; k < 5; k++) in.m_pld[k] = clampd(u[(FB_U_M_PILOT + k) * stride], 0, 100);
    in.ui = ui;
}
// quantities f_step! reads from the y of the last f_ode! (aircraftbase.jl:172-181; c172.jl:715-724)
struct StepAux {
    real alpha;       // aero.y.α (c172.jl:375-384)
    real m_avail;     // fuel.y.m_avail (c172.jl:641)
    int wow;            // bit g: strut g weight-on-wheel (landinggear.jl:479-483)
    int crash;          // bit g: strut g has α_ts > 60° or -ξ_dot > 10, i.e. its f_step! throws GroundCrash (landinggear.jl:331-347)
};

// accumulate point mass into (m, m r, J)  (dynamics.jl:211-214)
FBD void add_point(real m, const real* r, real& M, v3& Mr, real (&J)[6]) {
    M += m;
    Mr = Mr + m * v3{r[0], r[1], r[2]};
    J[0] += m * (r[1] * r[1] + r[2] * r[2]);
    J[1] += m * (r[0] * r[0] + r[2] * r[2]);
    J[2] += m * (r[0] * r[0] + r[1] * r[1]);
    J[3] -= m * (r[0] * r[1]);  // xy
    J[4] -= m * (r[0] * r[2]);  // xz
    J[5] -= m * (r[1] * r[2]);  // yz
}
template <class InA>
FBD void sum_payload_of(InA& in) {
    real M = 0, J[6] = {0, 0, 0, 0, 0, 0};
    v3 Mr = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 5; k++) add_point(in.get_m_pld(k), c172::pld_r[k], M, Mr, J);
    in.pld_M = M; in.pld_Mr[0] = Mr.x; in.pld_Mr[1] = Mr.y; in.pld_Mr[2] = Mr.z;
#pragma unroll
    for (int k = 0; k < 6; k++) in.pld_J[k] = J[k];
}
// total mass properties at Ob (dynamics.jl:328-399; c172.jl:26-44, 542-554, 618-636): airframe + fuel + payload, then the CoM and
// the inertia about it (Jc = xx yy zz xy xz yz)
template <class In>
FBD void mass_props(real m_fuel_total, const In& in, real& M, real (&J)[6], real& iM, v3& r_bc, real (&Jc)[6]) {
    using namespace c172;
    M = afm_m;
    J[0] = afm_J[0] + afm_m * (afm_r[1] * afm_r[1] + afm_r[2] * afm_r[2]);
    J[1] = afm_J[1] + afm_m * (afm_r[0] * afm_r[0] + afm_r[2] * afm_r[2]);
    J[2] = afm_J[2] + afm_m * (afm_r[0] * afm_r[0] + afm_r[1] * afm_r[1]);
    J[3] = -afm_m * (afm_r[0] * afm_r[1]); J[4] = -afm_m * (afm_r[0] * afm_r[2]); J[5] = -afm_m * (afm_r[1] * afm_r[2]);
    v3 Mr = afm_m * v3{afm_r[0], afm_r[1], afm_r[2]};
    const real m_half = FBL(0.5) * fmax(FBL(0.0), m_fuel_total);
    // the two half-masses sit at (0.325, -/+2.845, 0) (c172.jl:628-629): their sums of r, r r' are compile-time constants,
    // so both tanks together are one multiply-add per non-zero component
    {
        constexpr real sx = fuel_r[0][0] + fuel_r[1][0], sy = fuel_r[0][1] + fuel_r[1][1], sz = fuel_r[0][2] + fuel_r[1][2];
        constexpr real j0 = fuel_r[0][1] * fuel_r[0][1] + fuel_r[0][2] * fuel_r[0][2] + fuel_r[1][1] * fuel_r[1][1] + fuel_r[1][2] * fuel_r[1][2];
        constexpr real j1 = fuel_r[0][0] * fuel_r[0][0] + fuel_r[0][2] * fuel_r[0][2] + fuel_r[1][0] * fuel_r[1][0] + fuel_r[1][2] * fuel_r[1][2];
        constexpr real j2 = fuel_r[0][0] * fuel_r[0][0] + fuel_r[0][1] * fuel_r[0][1] + fuel_r[1][0] * fuel_r[1][0] + fuel_r[1][1] * fuel_r[1][1];
        constexpr real j3 = fuel_r[0][0] * fuel_r[0][1] + fuel_r[1][0] * fuel_r[1][1], j4 = fuel_r[0][0] * fuel_r[0][2] + fuel_r[1][0] * fuel_r[1][2];
        constexpr real j5 = fuel_r[0][1] * fuel_r[0][2] + fuel_r[1][1] * fuel_r[1][2];
        M += 2 * m_half;
        if constexpr (sx != 0) Mr.x += m_half * sx;
        if constexpr (sy != 0) Mr.y += m_half * sy;
        if constexpr (sz != 0) Mr.z += m_half * sz;
        J[0] += m_half * j0; J[1] += m_half * j1; J[2] += m_half * j2;
        if constexpr (j3 != 0) J[3] -= m_half * j3;
        if constexpr (j4 != 0) J[4] -= m_half * j4;
        if constexpr (j5 != 0) J[5] -= m_half * j5;
    }
    if constexpr (In::pld_precomputed) {
        M += in.get_pld_M(); Mr = Mr + v3{in.get_pld_Mr(0), in.get_pld_Mr(1), in.get_pld_Mr(2)};
#pragma unroll
        for (int k = 0; k < 6; k++) J[k] += in.get_pld_J(k);
    } else {
#pragma unroll
        for (int k = 0; k < 5; k++) add_point(in.get_m_pld(k), pld_r[k], M, Mr, J);
    }
    iM = 1 / M;
    r_bc = iM * Mr;
    // inertia about the CoM: J_c = J_b + m skew(r)^2
    const real rr = dot(r_bc, r_bc);
    Jc[0] = J[0] - M * (rr - r_bc.x * r_bc.x); Jc[1] = J[1] - M * (rr - r_bc.y * r_bc.y); Jc[2] = J[2] - M * (rr - r_bc.z * r_bc.z);
    Jc[3] = J[3] + M * (r_bc.x * r_bc.y); Jc[4] = J[4] + M * (r_bc.x * r_bc.z); Jc[5] = J[5] + M * (r_bc.y * r_bc.z);
}

// the deflection-only parts of the aerodynamic coefficients (InputsAgg::sum_aero), as rhs() takes them from its inputs at the start
// of the aerodynamics block (fetch_aero: register copies for InputsAgg, loads from memory for inputs that park them there)
struct AeroC {
    loc l_df4, l_df2;
    real cd_in, cd_df, cy_in, cl_in, cl_df, croll_in, cm_in, cn_in;
};
// Inputs plus the payload's contribution to (m, m r, J): the five payload masses are constant over a launch, so the stepping
// kernels sum their point-mass terms once (10 numbers that then ride in AGPRs) instead of 40 fma's and as many constants per RHS.
struct InputsAgg : Inputs {
    static constexpr bool pld_precomputed = true, aero_precomputed = true;
    real pld_M, pld_J[6];
    real pld_Mr[3];
    FBD real get_pld_M() const { return pld_M; }
    FBD real get_pld_Mr(int k) const { return pld_Mr[k]; }
    FBD real get_pld_J(int k) const { return pld_J[k]; }
    FBD void fetch_aero(AeroC& c) const {
        c.l_df4 = l_df4; c.l_df2 = l_df2;
        c.cd_in = cd_in; c.cd_df = cd_df; c.cy_in = cy_in; c.cl_in = cl_in; c.cl_df = cl_df; c.croll_in = croll_in; c.cm_in = cm_in; c.cn_in = cn_in;
    }
    // the parts of the six aerodynamic coefficients that depend on the surface deflections alone (mechanical actuation: constant
    // over a launch), and the flap-axis table locations the mixed lookups need
    loc l_df4, l_df2;
    real cd_in, cd_df, cy_in, cl_in, cl_df, croll_in, cm_in, cn_in;
    FBD void sum_aero(lds_cptr A, lds_cptr RA) {
        auto S_ = [&](int k) -> real { return A[AT_SCALARS + k]; };
        l_df4 = grid_locate<4>(A + AT_DF4_K, RA + AT_DF4_K, this->df, true, true);
        l_df2 = grid_locate<2>(A + AT_DF2_K, RA + AT_DF2_K, this->df, true, true);
        const loc l_de = grid_locate<3>(A + AT_UNIT3_K, RA + AT_UNIT3_K, this->de, true, true);
        cd_in = S_(AS_CD_ZERO) + lerp1(A + AT_CD_DE_V, l_de);
        cd_df = lerp1(A + AT_CD_DF_V, l_df4);
        cy_in = S_(AS_CY_DR) * this->dr + S_(AS_CY_DA) * this->da;
        cl_in = S_(AS_CL_DE) * this->de;
        cl_df = lerp1(A + AT_CL_DF_V, l_df4);
        croll_in = S_(AS_Cl_DA) * this->da + S_(AS_Cl_DR) * this->dr;
        cm_in = S_(AS_CM_ZERO) + S_(AS_CM_DE) * this->de + lerp1(A + AT_CM_DF_V, l_df4);
        cn_in = S_(AS_CN_DR) * this->dr + S_(AS_CN_DA) * this->da;
    }
    FBD void sum_payload() { sum_payload_of(*this); }
    // ground-only inputs (nose-wheel steering, brakes), fetched once per launch by the ground-capable stepper instead of from global
    // memory inside every contact evaluation (three exposed L2 round trips per RHS on the ground)
    real steer_in, brake_l, brake_r;
    FBD void load_ground_inputs() { steer_in = Inputs::get_steering(); brake_l = Inputs::get_brake(0); brake_r = Inputs::get_brake(1); }
    FBD real get_steering() const { return steer_in; }
    FBD real get_brake(int g) const { return g == 0 ? brake_l : brake_r; }
};

// Ground-contact branch of one landing-gear unit (landinggear.jl:260-328, 426-476). Rare and divergent:
// kept out of line so that the airborne path does not pay its registers.
struct GroundIn {
    quat q_eb, q_nb, q_en;
    v3 r_eb_e, r_bs_e, ks_e, w_eb_b, v_eb_b, loc_Ot;
    v3 ut_e;          // the terrain normal (local vertical) in ECEF axes, and its projection on the strut axis: the same for the three
    real ut_ks;       // units, formed once per evaluation by ground_common()
    real he_Ot, frc_out0, frc_out1, steer_in, brake_in;
    int g, steer_engaged, surface;
    lds_cptr atan_tab;   // the stepping kernels' atan table (FAST forms)
};
struct GroundOut {
    v3 F_b, tau_b;
    real v_xy0, v_xy1, xi, xi_dot, F_dmp;
    quat q_sc;   // strut -> contact frame rotation, kept between the two phases
    v3 r_bc_b;   // contact point in body frame
    int st;
};
// What the three units share (landinggear.jl:262-275): q_en, the strut axis and the terrain normal in ECEF axes, the tilt angle between
// them and its crash criterion (> 60 degrees: the strut's GroundCrash, :331-338). FAST (the stepping kernels): the criterion is decided
// on the cosine — acos is evaluated only for a lane within 1e-7 of cos 60 degrees, where the rounding of acos(x) 180 / pi decides.
struct GroundCommon { quat q_en; v3 ks_e, ut_e; real ut_ks, alpha_ts; bool tilt_crash; };
template <bool FAST> __device__ __forceinline__ void ground_common(quat q_eb, quat q_en, GroundCommon& c);
// FAST = the stepping kernels' forms (see c172_kernels.hpp); !FAST = the reference's operations one by one (f_ode!, the output record)
template <bool FAST> __device__ __forceinline__ void gear_ground_kinematics(const GroundIn& in, GroundOut& o);
template <bool FAST> __device__ __forceinline__ void gear_ground_force(const GroundIn& in, GroundOut& o);

// ---------------------------------------------------------------------------------------------
// One RHS evaluation. x[27] -> 27 derivatives through emit(); fills aux (for f_step!) and, if Y != nullptr, the output record.
// Call order of the reference: world.jl:26-32 -> aircraftbase.jl:221-230,142-170 -> c172.jl:697-713.
// Every derivative component is handed to `emit(index, value)` the moment it is known, so that the
// caller can consume it at once (the stepping kernel folds it into the RK stage sums in LDS) instead of
// keeping a 27-double array alive across the whole evaluation.
// Output sinks: where the components of the output record y go.
//   NoSink    — nowhere (the stepping kernel): everything that only feeds y is dead code;
//   PanelSink — the full record into a global [FB_NY x n] panel (f_ode!, logging);
//   a partial sink (enabled, !full) picks a few components — the control laws' inputs — and still allows the
//   shortcuts that a full record forbids.
template <class S, class = void> struct SinkDynamic : std::false_type {};
template <class S> struct SinkDynamic<S, std::void_t<typename S::dynamic_tag>> : std::true_type {};
template <class S> FBD bool sink_on(const S& s) { if constexpr (SinkDynamic<S>::value) return s.on; else return true; }
struct NoSink {
    static constexpr bool enabled = false, full = false;
    FBD void put(int, real) const {}
};
// emit functors may offer batch<NE>(j0, k): NE consecutive rows at once (all panel reads, then all updates, then all writes — the
// row-by-row form cannot overlap its LDS round trips, because the compiler must assume that one row's write through the
// stage-selected panel pointer aliases the next row's read). Functors without it get the rows one by one.
template <class E, class = void> struct EmitBatched : std::false_type {};
template <class E> struct EmitBatched<E, std::void_t<typename E::batched_tag>> : std::true_type {};
template <int NE, class Emit>
FBD void emit_rows(Emit& emit, int j0, const real (&k)[NE]) {
    if constexpr (EmitBatched<typename std::remove_reference<Emit>::type>::value) emit.template batch<NE>(j0, k);
    else {
#pragma unroll
        for (int e = 0; e < NE; e++) emit(j0 + e, k[e]);
    }
}
// Gravity at the CoM in body axes, along -n_e(Oc) (dynamics.jl:476-488). The reference converts r_ec_e = r_eb_e + q_eb(r_bc) back to
// geodetic coordinates (Fukushima, ~210 instructions here) and builds ltf(Oc) from it (~140 more). Oc is within a metre
// of Ob, whose geodetic coordinates are the kinematic state, so the conversion is done as a first-order expansion about
// Ob instead: neglected terms are |r_bc|^2 / R ~ 1e-7 m in h_c and ~1e-14 in n_c. One subtlety is kept to first order:
// at RK stages the state n-vector u = n_e is off unit norm by eps ~ 1e-8 (it is only renormalised in f_step!), and
// r_eb_e is built from that u, which puts Ob eps (R_E + h) ~ 6 cm higher and eps e^2 R_N sin(2 lat) / 2(1 - e^2) further
// north than (u / |u|, h_e); both shifts are added before the expansion.
// Geodetic coordinates of the point Ob + d_e (d_e in ECEF axes, a few metres), expanded about Ob = (n_e, h_e) — see gravity_com.
// SECOND adds the second-order terms (the curvature of the ellipsoid under the tangential offset: 4e-7 m in altitude at 2.3 m, and
// the same amount through the length of n_c): with them the result is within |d|^3 / R^2 ~ 1e-13 m of the exact conversion. dlat / dlon: the point's latitude / longitude minus
// those of n_e / |n_e|.
template <bool SECOND>
FBD void offset_geodetic(v3 d_e, v3 n_e, real h_e, real R_N, real R_E, real i_RN, real i_RE, v3& n_c, real& h_c, real& dlat, real& dlon) {
    const real eps = FBL(0.5) * (dot(n_e, n_e) - 1);
    const v3 nh = (1 - eps) * n_e;
    const real p2 = nh.x * nh.x + nh.y * nh.y;
    const bool off_pole = p2 > FBL(1e-24);
    const real ip = off_pole ? rsqrt(p2) : FBL(0.0);
    const v3 e_E = off_pole ? v3{-nh.y * ip, nh.x * ip, FBL(0.0)} : v3{FBL(0.0), FBL(1.0), FBL(0.0)};
    const v3 e_N = cross(nh, e_E);
    const real up = dot(nh, d_e);
    const v3 d_t = d_e - up * nh;
    const real dN = dot(d_t, e_N) - eps * (wgs::e2 / (1 - wgs::e2)) * R_N * (nh.z * (p2 * ip));
    const real dE = dot(d_t, e_E);
    dlat = dN * i_RN;
    dlon = (dE * i_RE) * ip;
    n_c = nh + dlat * e_N + (dE * i_RE) * e_E;
    h_c = h_e + up + eps * (R_E + h_e);
    if constexpr (SECOND) {
        h_c += FBL(0.5) * (dN * dlat + dE * (dE * i_RE));
        // and n_c back to unit length: whoever builds an ECEF position from it multiplies its norm error (theta^2 / 2 ~ 6e-14) by the
        // Earth's radius (4e-7 m)
        const real th2 = dlat * dlat + (dE * i_RE) * (dE * i_RE);
        n_c = (1 - FBL(0.5) * th2) * n_c;
    }
}
FBD v3 gravity_com(quat q_eb, v3 r_bc, v3 n_e, real h_e, real R_N, real R_E, real i_RN, real i_RE, int32_t& st, v3& d_e) {
    d_e = qrot(q_eb, r_bc);
    v3 n_c;
    real h_c, dlat, dlon;
    offset_geodetic<false>(d_e, n_e, h_e, R_N, R_E, i_RN, i_RE, n_c, h_c, dlat, dlon);
    if (!(h_c >= H_MIN)) st |= FB_ST_ALT_RANGE;
    const real g = normal_gravity(n_c.z, h_c);
    // g_c = q_cl(0,0,g) with q_cl = q_eb' ∘ ltf(Oc). ltf(Oc) maps the local down axis to -n_c exactly, so the rotated vector
    // is w_g = -g n_c; what remains is the rotation by q_eb', whose norm s is off 1 by ~1e-8 at RK stages. The reference's
    // v + 2 q_im x (q_re v + q_im x v) evaluates to (1 - s^2) v + s^2 R v, applied there to (0,0,g) with the composed q_cl and
    // here to w_g with q_eb' alone: the difference (1 - s^2)((0,0,g) - w_g) ~ 4e-7 m/s^2 is added back explicitly.
    const v3 w_g = (-g) * n_c;
    const real s2 = q_eb.w * q_eb.w + q_eb.x * q_eb.x + q_eb.y * q_eb.y + q_eb.z * q_eb.z;
    return qrot(qconj(q_eb), w_g) + (1 - s2) * (v3{FBL(0.0), FBL(0.0), g} - w_g);
}
// q_eb'(0, 0, w_ie): the Earth rate in body axes — the rotation formula written out for a vector along z (a third of the generic form's operations)
FBD v3 earth_rate_b(quat q_eb) {
    return {(2 * wgs::w_ie) * (q_eb.x * q_eb.z - q_eb.w * q_eb.y), (2 * wgs::w_ie) * (q_eb.y * q_eb.z + q_eb.w * q_eb.x),
            wgs::w_ie * (1 - 2 * (q_eb.x * q_eb.x + q_eb.y * q_eb.y))};
}
struct PanelSink {
    static constexpr bool enabled = true, full = true;
    double* Y;   // &y[0 * n + i]
    int64_t n;
    FBD void put(int k, real v) const { __builtin_nontemporal_store((double)v, &Y[(int64_t)k * n]); }   // a 1.4 KB/aircraft stream nobody re-reads on the device: keep it out of L2
};
// GROUND = false compiles the landing gear's ground-contact branch (and the three per-wheel geodetic conversions) out: such an
// instance can only evaluate states in the high-clearance regime and answers FB_ST_INTERNAL_REDO anywhere else, so that the
// caller repeats the work with the full instance (k_step_air: the airborne pass, then a GROUND = true pass over the lanes that asked for it).
constexpr int32_t FB_ST_INTERNAL_REDO = 1 << 30;
// SCALAR_KNOTS: knot scans of the gridded tables read the fp64 blob in global memory (uniform addresses -> scalar loads) instead of LDS.
template <int KIN, bool GROUND = true, bool SCALAR_KNOTS = false, class Sink, class Emit, class In, class XV>
FBD int32_t rhs(const XV& x, int stall, int eng_state, const In& in, const Env& env, const Tables& T,
                Emit&& emit, StepAux& aux, Sink&& sink) {
    using namespace c172;
    using SinkT = typename std::remove_reference<Sink>::type;
    // (a sink with a run-time switch — SinkT::dynamic, sink.on: the stepping kernels' tap, wave-uniform — makes the output blocks run-time branches of ONE
    // instance of this function; every other sink decides at compile time, as before)
    const bool WITH_Y = SinkT::enabled && sink_on(sink);
    constexpr int NC = SinkT::full ? PR_NC : PR_NC_STEP;   // propeller table stride in LDS (see stage_tables)
    auto gkp = [&](int off) -> gk_cptr { return SCALAR_KNOTS ? T.gk + off : nullptr; };
    int32_t st = 0;
    PHASE_FENCE(0);
    auto YP = [&](int k, real v) { if (WITH_Y) sink.put(k, v); };
    auto YP3 = [&](int k, v3 v) { if (WITH_Y) { sink.put(k, v.x); sink.put(k + 1, v.y); sink.put(k + 2, v.z); } };
    auto YP4 = [&](int k, quat q) { if (WITH_Y) { sink.put(k, q.w); sink.put(k + 1, q.x); sink.put(k + 2, q.y); sink.put(k + 3, q.z); } };

    // ===== kinematics (FlightPhysics/src/kinematics.jl): WA :181-223, ECEF :282-320, NED :366-407 =====
    // Rows FB_X_Q_WB.. hold the mechanisation's own states: WA q_wb[4] q_ew[4] h_e; ECEF q_eb[4] n_e[3] h_e (one row unused);
    // NED ψ θ φ ϕ λ h_e (three rows unused; unused rows carry a zero derivative).
    constexpr int KX = FB_X_Q_WB;
    constexpr bool FASTM = SCALAR_KNOTS;   // the stepping kernels' own atan2 / log / sincos (the fp64 ones stage the atan table)
    const v3 w_eb_b = {x[FB_X_OMEGA_EB_B], x[FB_X_OMEGA_EB_B + 1], x[FB_X_OMEGA_EB_B + 2]};
    const v3 v_eb_b = {x[FB_X_V_EB_B], x[FB_X_V_EB_B + 1], x[FB_X_V_EB_B + 2]};
    const real h_e = x[KIN == FB_KIN_WA ? KX + 8 : (KIN == FB_KIN_ECEF ? KX + 7 : KX + 5)];
    if (!(h_e >= H_MIN)) st |= FB_ST_ALT_RANGE;
    quat q_nb, q_eb, q_en = {1, 0, 0, 0}, q_nw = {1, 0, 0, 0};
    v3 n_e;
    [[maybe_unused]] quat q_wb = {1, 0, 0, 0}, q_ew = {1, 0, 0, 0};   // (WA)
    [[maybe_unused]] real ned_s2 = 0, ned_c2 = 1, ned_s3 = 0, ned_c3 = 1, ned_cla = 1;   // (NED: sin, cos of θ/2 and φ/2, cos of the latitude state)
    if constexpr (KIN == FB_KIN_WA) {
        q_wb = {x[KX], x[KX + 1], x[KX + 2], x[KX + 3]};
        q_ew = {x[KX + 4], x[KX + 5], x[KX + 6], x[KX + 7]};
        // ψ_nw and n_e straight from q_ew (geodesy.jl:62-69, 140-147)
        const real dq12 = 2 * q_ew.w * q_ew.x, dq13 = 2 * q_ew.w * q_ew.y;
        const real dq24 = 2 * q_ew.x * q_ew.z, dq34 = 2 * q_ew.y * q_ew.z;
        n_e = {-(dq24 + dq13), -(dq34 - dq12), -(1 - 2 * (q_ew.x * q_ew.x + q_ew.y * q_ew.y))};
        // q_nw = Rz(ψ_nw), ψ_nw = atan2(-(dq34+dq12), dq24-dq13): only cos, sin of ψ_nw/2 are needed
        real s_nw, c_nw;
        half_angle_cs(-(dq34 + dq12), dq24 - dq13, c_nw, s_nw);
        q_nw = {c_nw, FBL(0.0), FBL(0.0), s_nw};
        q_nb = {c_nw * q_wb.w - s_nw * q_wb.z, c_nw * q_wb.x - s_nw * q_wb.y,    // qmul(q_nw, q_wb) without the products by q_nw's two zeros
                c_nw * q_wb.y + s_nw * q_wb.x, c_nw * q_wb.z + s_nw * q_wb.w};
        q_eb = qmul(q_ew, q_wb);
    } else if constexpr (KIN == FB_KIN_ECEF) {
        q_eb = {x[KX], x[KX + 1], x[KX + 2], x[KX + 3]};
        n_e = {x[KX + 4], x[KX + 5], x[KX + 6]};   // state n-vector, normalised only in f_step! (kinematics.jl:286, 317-320)
        q_en = ltf_quat(n_e);
        q_nb = qmul(qconj(q_en), q_eb);
    } else {
        real s1, c1, s3, c3, sla, slo, clo;
        if constexpr (FASTM) {
            sincos_step(FBL(0.5) * x[KX], s1, c1); sincos_step(FBL(0.5) * x[KX + 1], ned_s2, ned_c2); sincos_step(FBL(0.5) * x[KX + 2], s3, c3);
            sincos_step(x[KX + 3], sla, ned_cla); sincos_step(x[KX + 4], slo, clo);
        } else {
            fb_sincos(FBL(0.5) * x[KX], &s1, &c1); fb_sincos(FBL(0.5) * x[KX + 1], &ned_s2, &ned_c2); fb_sincos(FBL(0.5) * x[KX + 2], &s3, &c3);
            fb_sincos(x[KX + 3], &sla, &ned_cla); fb_sincos(x[KX + 4], &slo, &clo);
        }
        ned_s3 = s3; ned_c3 = c3;
        // Rz(ψ) ∘ Ry(θ) ∘ Rx(φ) (attitude.jl:393-395): the two quaternion products without their terms in the factors' zeros
        const quat zy = {c1 * ned_c2, -(s1 * ned_s2), c1 * ned_s2, ned_c2 * s1};
        q_nb = {zy.w * c3 - zy.x * s3, zy.w * s3 + c3 * zy.x, c3 * zy.y + zy.z * s3, c3 * zy.z - zy.y * s3};
        n_e = {ned_cla * clo, ned_cla * slo, sla};                                       // geodesy.jl:97-101
        q_en = ltf_quat(n_e);
        q_eb = qmul(q_en, q_nb);
    }

    real lat, lon;
#ifdef FB_GROUND_REFERENCE_FORMS   // A/B builds: the stepping kernels' ground contact in the reference's operations (tools/ground_error_quantiles.py)
    constexpr bool GFAST = false;
#else
    constexpr bool GFAST = FASTM;
#endif
    auto atan2m = [&](real y, real x0) -> real { if constexpr (FASTM) return atan2_step(y, x0, T.rk + LDS_ATAN); else return atan2(y, x0); };
    auto atan2p = [&](real y, real x0) -> real { if constexpr (FASTM) return atan2_step<true>(y, x0, T.rk + LDS_ATAN); else return atan2(y, x0); };   // x0 >= 0, not both zero
    GeoidCell gcell;
    const real N_geoid = geoid_height<FASTM>(T, n_e, lat, lon, gcell);
    const real h_o = h_e - N_geoid;
    if (!(h_o >= H_MIN)) st |= FB_ST_ALT_RANGE;
    PHASE_FENCE(11);

    const v3 v_eb_n = qrot(q_nb, v_eb_b);
    // radii of curvature and ECEF position (geodesy.jl:125-129, 418-428)
    const real i_fden = rsqrt(1 - wgs::e2 * n_e.z * n_e.z);   // 1 / sqrt(1 - e^2 sin^2 lat)
    const real R_E = wgs::a * i_fden;
    const real R_N = (wgs::a * (1 - wgs::e2)) * (i_fden * i_fden * i_fden);
    const v3 r_eb_e = {(R_E + h_e) * n_e.x, (R_E + h_e) * n_e.y, (R_E * (1 - wgs::e2) + h_e) * n_e.z};
    // transport rate (kinematics.jl:232-242)
    const real RE_h = R_E + h_e, RN_h = R_N + h_e, i_REN = 1 / (RE_h * RN_h);   // both reciprocals from one division
    const real i_RE = RN_h * i_REN, i_RN = RE_h * i_REN;
    const v3 w_ew_n = {v_eb_n.y * i_RE, -v_eb_n.x * i_RN, FBL(0.0)};
    v3 w_wb_b;
    if constexpr (KIN == FB_KIN_WA) {
        // q_nw'(w_ew_n): a rotation about z by -psi_nw of a vector without z component (cos, sin of psi_nw from the half-angle pair)
        const real cpsi = q_nw.w * q_nw.w - q_nw.z * q_nw.z, spsi = 2 * (q_nw.w * q_nw.z);
        const v3 w_ew_w = {cpsi * w_ew_n.x + spsi * w_ew_n.y, cpsi * w_ew_n.y - spsi * w_ew_n.x, FBL(0.0)};
        const v3 w_ew_b = qrot_inv(q_wb, w_ew_w);
        w_wb_b = w_eb_b - w_ew_b;
        // q ⊗ (0, v) = (-q_im·v, q_re v + q_im x v); w_ew_w has no z component
        const quat a = {-(q_wb.x * w_wb_b.x + q_wb.y * w_wb_b.y + q_wb.z * w_wb_b.z),
                        q_wb.w * w_wb_b.x + (q_wb.y * w_wb_b.z - q_wb.z * w_wb_b.y),
                        q_wb.w * w_wb_b.y + (q_wb.z * w_wb_b.x - q_wb.x * w_wb_b.z),
                        q_wb.w * w_wb_b.z + (q_wb.x * w_wb_b.y - q_wb.y * w_wb_b.x)};
        const quat b2 = {-(q_ew.x * w_ew_w.x + q_ew.y * w_ew_w.y), q_ew.w * w_ew_w.x - q_ew.z * w_ew_w.y,
                         q_ew.w * w_ew_w.y + q_ew.z * w_ew_w.x, q_ew.x * w_ew_w.y - q_ew.y * w_ew_w.x};
        const real kq1[4] = {FBL(0.5) * a.w, FBL(0.5) * a.x, FBL(0.5) * a.y, FBL(0.5) * a.z};
        const real kq2[5] = {FBL(0.5) * b2.w, FBL(0.5) * b2.x, FBL(0.5) * b2.y, FBL(0.5) * b2.z, -v_eb_n.z};
        emit_rows<4>(emit, KX, kq1);
        emit_rows<5>(emit, KX + 4, kq2);
    } else if constexpr (KIN == FB_KIN_ECEF) {
        w_wb_b = w_eb_b - qrot_inv(q_nb, w_ew_n);
        const quat a = qmul(q_eb, quat{FBL(0.0), w_eb_b.x, w_eb_b.y, w_eb_b.z});   // Attitude.dt(q_eb, ω_eb_b)
        const v3 nd = qrot(q_en, cross(w_ew_n, v3{FBL(0.0), FBL(0.0), -FBL(1.0)}));           // kinematics.jl:309
        emit(KX, FBL(0.5) * a.w); emit(KX + 1, FBL(0.5) * a.x); emit(KX + 2, FBL(0.5) * a.y); emit(KX + 3, FBL(0.5) * a.z);
        emit(KX + 4, nd.x); emit(KX + 5, nd.y); emit(KX + 6, nd.z);
        emit(KX + 7, -v_eb_n.z);
        emit(KX + 8, FBL(0.0));
    } else {
        w_wb_b = w_eb_b - qrot_inv(q_nb, w_ew_n);
        // ω_en_n (kinematics.jl:413-425) with ϕ = LatLon(Ob).ϕ re-derived from n_e, like the reference
        // FASTM: the trigonometric functions of the states from the half-angle pairs at hand (sin 2a = 2 s c, cos 2a = c^2 - s^2), and
        // tan of the latitude re-derived from n_e as n_z / |n_xy| — the function of n_e that tan(atan2(n_z, |n_xy|)) is
        real tan_lat, sph, cph, tth, sec, i_cla;
        if constexpr (FASTM) {
            tan_lat = n_e.z * rsqrt(n_e.x * n_e.x + n_e.y * n_e.y);
            sph = 2 * (ned_s3 * ned_c3); cph = ned_c3 * ned_c3 - ned_s3 * ned_s3;
            const real sth = 2 * (ned_s2 * ned_c2), cth = ned_c2 * ned_c2 - ned_s2 * ned_s2;
            sec = FBL(1.0) / cth; tth = sth * sec;
            i_cla = FBL(1.0) / ned_cla;
        } else {
            tan_lat = tan(lat);
            fb_sincos(x[KX + 2], &sph, &cph);
            tth = tan(x[KX + 1]); sec = FBL(1.0) / cos(x[KX + 1]);
            i_cla = 0;
        }
        const v3 w_en_n = {w_ew_n.x, w_ew_n.y, -v_eb_n.y * tan_lat / (R_E + h_e)};
        const v3 w_nb_b = w_eb_b - qrot_inv(q_nb, w_en_n);
        emit(KX, sph * sec * w_nb_b.y + cph * sec * w_nb_b.z);                 // Attitude.dt(e_nb, ω_nb_b), attitude.jl:436-449
        emit(KX + 1, cph * w_nb_b.y - sph * w_nb_b.z);
        emit(KX + 2, w_nb_b.x + sph * tth * w_nb_b.y + cph * tth * w_nb_b.z);
        emit(KX + 3, -w_en_n.y);                                               // Geodesy.dt(ϕ_λ, ω_en_n), geodesy.jl:112-118
        if constexpr (FASTM) emit(KX + 4, w_en_n.x * i_cla); else emit(KX + 4, w_en_n.x / cos(x[KX + 3]));
        emit(KX + 5, -v_eb_n.z);
        emit(KX + 6, FBL(0.0)); emit(KX + 7, FBL(0.0)); emit(KX + 8, FBL(0.0));
    }
    if (WITH_Y) {
        if constexpr (KIN == FB_KIN_WA) q_en = qmul(q_eb, qconj(q_nb));
        if constexpr (KIN == FB_KIN_NED) {   // e_nb, ϕ_λ are the states themselves
            YP(FB_Y_KIN + 0, x[KX]); YP(FB_Y_KIN + 1, x[KX + 1]); YP(FB_Y_KIN + 2, x[KX + 2]);
            lat = x[KX + 3]; lon = x[KX + 4];
        } else {
            // Euler angles (attitude.jl:382-391)
            const real q1 = q_nb.w, q2 = q_nb.x, q3 = q_nb.y, q4 = q_nb.z;
            YP(FB_Y_KIN + 0, atan2m(2 * (q1 * q4 + q2 * q3), 1 - 2 * (q3 * q3 + q4 * q4)));   // (atan2m: the table form in the stepping kernels' tap, the library's in f_ode!)
            YP(FB_Y_KIN + 1, asin(fmin(fmax(2 * (q1 * q3 - q2 * q4), -FBL(1.0)), FBL(1.0))));
            YP(FB_Y_KIN + 2, atan2m(2 * (q1 * q2 + q3 * q4), 1 - 2 * (q2 * q2 + q3 * q3)));
        }
        YP4(FB_Y_KIN + 3, q_nb); YP4(FB_Y_KIN + 7, q_eb); YP4(FB_Y_KIN + 11, q_en);
        YP(FB_Y_KIN + 15, lat); YP(FB_Y_KIN + 16, lon); YP3(FB_Y_KIN + 17, n_e);
        YP(FB_Y_KIN + 20, h_e); YP(FB_Y_KIN + 21, h_o); YP3(FB_Y_KIN + 22, r_eb_e);
        YP3(FB_Y_KIN + 25, w_wb_b); YP3(FB_Y_KIN + 28, w_eb_b); YP3(FB_Y_KIN + 31, v_eb_b); YP3(FB_Y_KIN + 34, v_eb_n);
        const real v_gnd = norm(v_eb_n);
        YP(FB_Y_KIN + 37, v_gnd);
        const bool chi_ok = KIN == FB_KIN_NED || v_gnd > FBL(0.1);   // the NED mechanisation has no low-speed guard (kinematics.jl:395-396)
        YP(FB_Y_KIN + 38, chi_ok ? atan2m(v_eb_n.y, v_eb_n.x) : FBL(0.0));
        YP(FB_Y_KIN + 39, chi_ok ? atan2(-v_eb_n.z, sqrt(v_eb_n.x * v_eb_n.x + v_eb_n.y * v_eb_n.y)) : FBL(0.0));
    }

    PHASE_FENCE(1);
    // ===== air data (atmosphere.jl:269-283, 220-242) =====
    real T_air, p_air;
    real lnp_air;
    const real h_gp = h_o * wgs::a / (wgs::a + h_o);   // geopotential altitude
    isa_data<FASTM>(h_gp, env.T_sl, env.p_sl, T_air, p_air, lnp_air, st);
    // one rsqrt(T) serves 1/T (density), sqrt(T) (speed of sound), 1/a (tip Mach number) and (T_ISA/T)^1/2 (engine)
    const real rs_T = rsqrt(T_air), i_T = rs_T * rs_T;
    const real rho = (p_air * (1 / isa::R)) * i_T;
    constexpr real sqrt_gR = FBL(20.046795704052055);   // sqrt(1.4 * 287.05287)
    static_assert(sqrt_gR * sqrt_gR > isa::gamma * isa::R * (1 - FBL(1e-7)) && sqrt_gR * sqrt_gR < isa::gamma * isa::R * (1 + FBL(1e-7)), "sqrt(gamma R)");
    const real a_snd = sqrt_gR * (T_air * rs_T), i_a_snd = (1 / sqrt_gR) * rs_T;
    const v3 v_ew_n = {env.wind_n, env.wind_e, env.wind_d};
    const v3 v_ew_b = qrot_inv(q_nb, v_ew_n);
    const v3 v_wb_b = v_eb_b - v_ew_b;
    const real TAS = norm(v_wb_b);
    const real q_dyn = FBL(0.5) * rho * (TAS * TAS);
    if (WITH_Y) {
        YP3(FB_Y_AIR, v_ew_n); YP3(FB_Y_AIR + 3, v_ew_b); YP3(FB_Y_AIR + 6, v_wb_b);
        const real M = TAS / a_snd;
        const real Tt = T_air * (1 + (isa::gamma - 1) / 2 * (M * M));
        const real pt = p_air * pow(Tt / T_air, isa::gamma / (isa::gamma - 1));
        const real dp = pt - p_air;
        YP(FB_Y_AIR + 9, T_air); YP(FB_Y_AIR + 10, p_air); YP(FB_Y_AIR + 11, rho); YP(FB_Y_AIR + 12, a_snd);
        YP(FB_Y_AIR + 13, (isa::beta_s * pow(T_air, FBL(1.5))) / (T_air + isa::S));
        YP(FB_Y_AIR + 14, M); YP(FB_Y_AIR + 15, Tt); YP(FB_Y_AIR + 16, pt); YP(FB_Y_AIR + 17, dp); YP(FB_Y_AIR + 18, q_dyn);
        YP(FB_Y_AIR + 19, TAS); YP(FB_Y_AIR + 20, TAS * sqrt(rho / isa::rho_std));
        YP(FB_Y_AIR + 21, sqrt(2 * isa::gamma / (isa::gamma - 1) * isa::p_std / isa::rho_std *
                               (pow(1 + dp / isa::p_std, (isa::gamma - 1) / isa::gamma) - 1)));
    }

    v3 F_b = {0, 0, 0}, tau_b = {0, 0, 0};  // total external wrench at Ob, body axes

    PHASE_FENCE(2);
    // ===== aerodynamics (c172.jl:307-373, 226-245) =====
    {
        lds_cptr A = T.lds + LDS_AERO;
        lds_cptr RA = T.rk + LDS_AERO;
        [[maybe_unused]] AeroC ac;
        if constexpr (In::aero_precomputed) in.fetch_aero(ac);
        real alpha = 0, beta = 0, cos_al = 1, sin_al = 0;
        if (TAS > FBL(0.1)) {  // also covers get_airflow_angles' own ‖v‖ < 0.1 guard (atmosphere.jl:329-337)
            const real r2 = v_wb_b.x * v_wb_b.x + v_wb_b.z * v_wb_b.z;
            const bool r_ok = r2 > 0;
            const real ir = rsqrt(r_ok ? r2 : FBL(1.0)), r = r2 * ir;
            alpha = atan2m(v_wb_b.z, v_wb_b.x);
            beta = atan2p(v_wb_b.y, r);   // (TAS > 0.1: r and v_y are not both zero)
            if (r_ok) { cos_al = v_wb_b.x * ir; sin_al = v_wb_b.z * ir; }   // cos, sin of atan2(z, x) (atan2(0, 0) = 0)
        }
        const real V = fmax(TAS, V_min);
        const real afd = 1 / tau_filt * (alpha - x[FB_X_ALPHA_FILT]);
        const real bfd = 1 / tau_filt * (beta - x[FB_X_BETA_FILT]);
        const real kf2[2] = {afd, bfd};
        static_assert(FB_X_BETA_FILT == FB_X_ALPHA_FILT + 1, "filter rows are adjacent");
        emit_rows<2>(emit, FB_X_ALPHA_FILT, kf2);
        const real i2V = 1 / (2 * V);
        const real p_nd = w_wb_b.x * b * i2V, q_nd = w_wb_b.y * c * i2V, r_nd = w_wb_b.z * b * i2V;
        const real ad_nd = clampd(afd * c * i2V, -FBL(0.04), FBL(0.04));
        const real dh_nd = (h_o - env.h_trn) / b;
        const real al = clampd(alpha, -FBL(0.1), FBL(0.36)), be = clampd(beta, -FBL(0.2), FBL(0.2));

        const loc l_ge = grid_locate<13, SCALAR_KNOTS, AUX_GE>(A + AT_GE_K, RA + AT_GE_K, dh_nd, true, true, gkp(LDS_AERO + AT_GE_K), T.gk);
        const loc l_al26 = grid_locate<26, SCALAR_KNOTS, AUX_AL26>(A + AT_CD_ALPHA_K, RA + AT_CD_ALPHA_K, al, true, true, gkp(LDS_AERO + AT_CD_ALPHA_K), T.gk);
        const loc l_al17 = grid_locate<17, SCALAR_KNOTS, AUX_AL17>(A + AT_CL_ALPHA_K, RA + AT_CL_ALPHA_K, al, true, true, gkp(LDS_AERO + AT_CL_ALPHA_K), T.gk);
        const loc l_al2 = grid_locate<2, SCALAR_KNOTS>(A + AT_ALPHA2_K, RA + AT_ALPHA2_K, al, true, true, gkp(LDS_AERO + AT_ALPHA2_K));
        const loc l_be3 = grid_locate<3, SCALAR_KNOTS>(A + AT_CY_BETA_K, RA + AT_CY_BETA_K, be, true, true, gkp(LDS_AERO + AT_CY_BETA_K));
        const loc l_bu = grid_locate<3, SCALAR_KNOTS>(A + AT_UNIT3_K, RA + AT_UNIT3_K, be, true, true, gkp(LDS_AERO + AT_UNIT3_K));
        const loc l_stall = {0, stall ? FBL(1.0) : FBL(0.0)};
        PHASE_FENCE(12);
        // the twenty scalar derivatives: uniform addresses -> scalar loads when the global blob is available
        auto S_ = [&](int k) -> real { return SCALAR_KNOTS ? T.gk[LDS_AERO + AT_SCALARS + k] : A[AT_SCALARS + k]; };
        real C_D, C_Y, C_L, C_l, C_m, C_n;
        if constexpr (In::aero_precomputed) {   // (the deflection-only terms come summed with the inputs; same terms, different order of addition)
            const loc l_df4 = ac.l_df4, l_df2 = ac.l_df2;
            C_D = ac.cd_in + lerp1(A + AT_CD_GE_V, l_ge) * (lerp2(A + AT_CD_ALPHA_DF_V, 26, l_al26, l_df4) + ac.cd_df) + lerp1(A + AT_CD_BETA_V, l_bu);
            C_Y = ac.cy_in + lerp2(A + AT_CY_BETA_DF_V, 3, l_be3, l_df2) +
                  lerp2(A + AT_CY_P_V, 2, l_al2, l_df2) * p_nd + lerp2(A + AT_CY_R_V, 2, l_al2, l_df2) * r_nd;
            C_L = lerp1(A + AT_CL_GE_V, l_ge) * (lerp2(A + AT_CL_ALPHA_V, 17, l_al17, l_stall) + ac.cl_df) +
                  ac.cl_in + S_(AS_CL_Q) * q_nd + S_(AS_CL_ALPHA_DOT) * ad_nd;
            C_l = ac.croll_in + S_(AS_Cl_BETA) * be + S_(AS_Cl_P) * p_nd + lerp2(A + AT_CL_R_V, 2, l_al2, l_df2) * r_nd;
            C_m = ac.cm_in + S_(AS_CM_ALPHA) * al + S_(AS_CM_Q) * q_nd + S_(AS_CM_ALPHA_DOT) * ad_nd;
            C_n = ac.cn_in + S_(AS_CN_BETA) * be + S_(AS_CN_P) * p_nd + S_(AS_CN_R) * r_nd;
        } else {
            const real de = in.get_de(), da = in.get_da(), dr = in.get_dr(), df = in.get_df();
            const loc l_df4 = grid_locate<4, SCALAR_KNOTS>(A + AT_DF4_K, RA + AT_DF4_K, df, true, true, gkp(LDS_AERO + AT_DF4_K));
            const loc l_df2 = grid_locate<2, SCALAR_KNOTS>(A + AT_DF2_K, RA + AT_DF2_K, df, true, true, gkp(LDS_AERO + AT_DF2_K));
            const loc l_de = grid_locate<3, SCALAR_KNOTS>(A + AT_UNIT3_K, RA + AT_UNIT3_K, de, true, true, gkp(LDS_AERO + AT_UNIT3_K));
            C_D = S_(AS_CD_ZERO) + lerp1(A + AT_CD_GE_V, l_ge) * (lerp2(A + AT_CD_ALPHA_DF_V, 26, l_al26, l_df4) + lerp1(A + AT_CD_DF_V, l_df4)) +
                  lerp1(A + AT_CD_DE_V, l_de) + lerp1(A + AT_CD_BETA_V, l_bu);
            C_Y = S_(AS_CY_DR) * dr + S_(AS_CY_DA) * da + lerp2(A + AT_CY_BETA_DF_V, 3, l_be3, l_df2) +
                  lerp2(A + AT_CY_P_V, 2, l_al2, l_df2) * p_nd + lerp2(A + AT_CY_R_V, 2, l_al2, l_df2) * r_nd;
            C_L = lerp1(A + AT_CL_GE_V, l_ge) * (lerp2(A + AT_CL_ALPHA_V, 17, l_al17, l_stall) + lerp1(A + AT_CL_DF_V, l_df4)) +
                  S_(AS_CL_DE) * de + S_(AS_CL_Q) * q_nd + S_(AS_CL_ALPHA_DOT) * ad_nd;
            C_l = S_(AS_Cl_DA) * da + S_(AS_Cl_DR) * dr + S_(AS_Cl_BETA) * be + S_(AS_Cl_P) * p_nd +
                  lerp2(A + AT_CL_R_V, 2, l_al2, l_df2) * r_nd;
            C_m = S_(AS_CM_ZERO) + S_(AS_CM_DE) * de + lerp1(A + AT_CM_DF_V, l_df4) + S_(AS_CM_ALPHA) * al + S_(AS_CM_Q) * q_nd +
                  S_(AS_CM_ALPHA_DOT) * ad_nd;
            C_n = S_(AS_CN_DR) * dr + S_(AS_CN_DA) * da + S_(AS_CN_BETA) * be + S_(AS_CN_P) * p_nd + S_(AS_CN_R) * r_nd;
        }

        // stability -> body axes: rotation by Ry(-α) with the UNCLAMPED α (c172.jl:356-359; atmosphere.jl:353-356)
        // (as a matrix, from cos α = x/r, sin α = z/r: the reference's quaternion form needs sincos(α/2), a hundred instructions)
        const real qS = q_dyn * S;
        const v3 F_s = {qS * -C_D, qS * C_Y, qS * -C_L};
        const v3 F_a = {cos_al * F_s.x - sin_al * F_s.z, F_s.y, sin_al * F_s.x + cos_al * F_s.z};
        const v3 tau_a = {qS * (C_l * b), qS * (C_m * c), qS * (C_n * b)};
        F_b = F_b + F_a;
        tau_b = tau_b + tau_a;
        aux.alpha = alpha;
        if (WITH_Y) {
            YP(FB_Y_AERO, alpha); YP(FB_Y_AERO + 1, beta); YP(FB_Y_AERO + 2, afd); YP(FB_Y_AERO + 3, bfd);
            YP(FB_Y_AERO + 4, C_D); YP(FB_Y_AERO + 5, C_Y); YP(FB_Y_AERO + 6, C_L); YP(FB_Y_AERO + 7, C_l); YP(FB_Y_AERO + 8, C_m); YP(FB_Y_AERO + 9, C_n);
            YP3(FB_Y_AERO + 10, F_a); YP3(FB_Y_AERO + 13, tau_a);
        }
    }

    PHASE_FENCE(3);
    // ===== landing gear: left, right, nose (landinggear.jl:524-537, 228-328, 411-476) =====
    aux.wow = 0;
    aux.crash = 0;
    // High-clearance shortcut (exact for the state): every strut attachment is within 2.3 m of Ob and the geoid
    // moves by < 1 mm over that distance, so when Ob is more than 10 m above the terrain no wheel can touch it:
    // wow = false, zero wrench, regulator input 0 (landinggear.jl:255-258, 418-424) without evaluating the three
    // ECEF->geodetic conversions and geoid gathers. Not taken when the FULL output record (which logs Δh) is requested.
    static_assert(GROUND || !SinkT::full, "the full output record needs the ground-capable instance");
    // Nor within 10 m of the altitude floor h_min: there the wheels' own ellipsoidal altitudes decide whether — and at which evaluation —
    // Geographic(r_ew0_e) throws (landinggear.jl:240 -> geodesy.jl:218-221), so they are evaluated.
    const bool clear10 = !SinkT::full && (fmin(h_o - env.h_trn, h_e - H_MIN) > FBL(10.0));
    if (!GROUND && !clear10) st |= FB_ST_INTERNAL_REDO;
    const bool high_clearance = GROUND ? clear10 : true;
    [[maybe_unused]] GroundCommon gcm;
    if constexpr (GROUND) {
        gcm.tilt_crash = false; gcm.alpha_ts = 0;
        // kinematics.y.q_en as each mechanisation defines it: WA q_eb ∘ q_nb' (kinematics.jl:195 — off unit norm by |q_wb|^2 at RK stages,
        // which the strut geometry then sees), ECEF and NED ltf(n_e) itself (:293, :377)
        if (!high_clearance) ground_common<GFAST>(q_eb, KIN == FB_KIN_WA ? qmul(q_eb, qconj(q_nb)) : q_en, gcm);
    }
#pragma unroll
    for (int g = 0; g < 3; g++) {
        PHASE_FENCE(4);
        v3 r_bs_e = {0, 0, 0}, loc_Ot = {1, 0, 0};
        real he_Ot = 0, dh = 0;
        bool wow = false;
        if (!high_clearance) {
            const v3 r_bs_b = {ldg_r[g][0], ldg_r[g][1], ldg_r[g][2]};
            r_bs_e = qrot(q_eb, r_bs_b);
            // The wheel's geodetic coordinates (the reference converts r_ew0_e = r_eb_e + r_bs_e back with Fukushima's method and looks
            // the geoid up again, landinggear.jl:240-258): the wheel is within 2.3 m of Ob, whose geodetic coordinates are the
            // kinematic state, so they come from the second-order expansion about Ob (1e-13 m from the exact conversion, 45
            // instructions instead of 210) and the geoid from the cell Ob's own lookup has already fetched (25 instead of 150).
            real he_Ow0, dlat_w, dlon_w;
            offset_geodetic<true>(r_bs_e, n_e, h_e, R_N, R_E, i_RN, i_RE, loc_Ot, he_Ow0, dlat_w, dlon_w);
            if (!(he_Ow0 >= H_MIN)) st |= FB_ST_ALT_RANGE;
            he_Ot = env.h_trn + geoid_height_near(T, gcell, dlat_w, dlon_w);
            dh = he_Ow0 - he_Ot;
            wow = dh <= 0;
        }
        const real x0 = x[FB_X_LDG_FRC + 2 * g], x1 = x[FB_X_LDG_FRC + 2 * g + 1];
        real v_xy0 = 0, v_xy1 = 0;
        GroundOut go;
        go.F_b = {0, 0, 0}; go.tau_b = {0, 0, 0}; go.xi = 0; go.xi_dot = 0; go.F_dmp = 0; go.st = 0;
        GroundIn gi;
        if constexpr (GROUND) if (wow) {
            gi.q_eb = q_eb; gi.q_nb = q_nb; gi.q_en = gcm.q_en;
            gi.r_eb_e = r_eb_e; gi.r_bs_e = r_bs_e; gi.ks_e = gcm.ks_e; gi.ut_e = gcm.ut_e; gi.ut_ks = gcm.ut_ks;
            gi.atan_tab = T.rk + LDS_ATAN;
            gi.w_eb_b = w_eb_b; gi.v_eb_b = v_eb_b; gi.loc_Ot = loc_Ot; gi.he_Ot = he_Ot;
            gi.g = g; gi.surface = env.surface;
            gi.steer_engaged = (in.ui & FB_UI_STEERING_ENGAGED) ? 1 : 0;
            // ground-only inputs, fetched on demand (c172s.jl:107-110; c172x.jl:139-141)
            gi.steer_in = (g == 2) ? in.get_steering() : FBL(0.0);
            gi.brake_in = (g == 2) ? FBL(0.0) : in.get_brake(g);
            gear_ground_kinematics<GFAST>(gi, go);
            v_xy0 = go.v_xy0; v_xy1 = go.v_xy1;
            st |= go.st;
        }
        // friction regulator: input = -v_ec_xy (zero when airborne) (landinggear.jl:418-424)
        real out0, out1;
        emit(FB_X_LDG_FRC + 2 * g, pi_ode(frc_kp, frc_ki, frc_kl, -FBL(1.0), FBL(1.0), -v_xy0, x0, out0));
        emit(FB_X_LDG_FRC + 2 * g + 1, pi_ode(frc_kp, frc_ki, frc_kl, -FBL(1.0), FBL(1.0), -v_xy1, x1, out1));
        if constexpr (GROUND) if (wow) {
            gi.frc_out0 = out0; gi.frc_out1 = out1;
            gear_ground_force<GFAST>(gi, go);
            F_b = F_b + go.F_b;
            tau_b = tau_b + go.tau_b;
            aux.wow |= (1 << g);
            if (gcm.tilt_crash) aux.crash |= (1 << g);
        }
        if (-go.xi_dot > 10) aux.crash |= (1 << g);
        if (WITH_Y) {
            const int k = FB_Y_LDG + 11 * g;
            YP(k, dh); YP(k + 1, wow ? FBL(1.0) : FBL(0.0)); YP(k + 2, go.xi); YP(k + 3, go.xi_dot); YP(k + 4, go.F_dmp);
            YP3(k + 5, go.F_b); YP3(k + 8, go.tau_b);
        }
    }

    PHASE_FENCE(6);
    // ===== fuel mass (c172.jl:607-616) and total mass properties at Ob (dynamics.jl:328-399; c172.jl:26-44, 542-554, 618-636) =====
    // (they depend on the state alone; the fuel row itself is emitted behind the engine, which supplies the fuel flow)
    const real m_fuel_total = m_res + x[FB_X_FUEL] * (m_full - m_res);
    aux.m_avail = m_fuel_total - m_res;
    YP(FB_Y_FUEL, m_fuel_total);

    PHASE_FENCE(7);
    real M = afm_m, iM = 0;
    v3 r_bc = {0, 0, 0};   // CoM position in body frame
    real J[6] = {0, 0, 0, 0, 0, 0};
    real Jxx = 0, Jyy = 0, Jzz = 0, Jxy = 0, Jxz = 0, Jyz = 0;   // inertia about the CoM
    {
        real Jc[6];
        mass_props(m_fuel_total, in, M, J, iM, r_bc, Jc);
        Jxx = Jc[0]; Jyy = Jc[1]; Jzz = Jc[2]; Jxy = Jc[3]; Jxz = Jc[4]; Jyz = Jc[5];
    }

    PHASE_FENCE(5);
    // ===== power plant: propeller then engine (piston.jl:575-595; propellers.jl:405-452; piston.jl:314-426) =====
    v3 h_rot = {0, 0, 0};
    real mdot = 0;
    {
        lds_cptr PT = T.lds + LDS_PISTON;
        lds_cptr RPT = T.rk + LDS_PISTON;
        lds_cptr PR = T.lds + LDS_PROP;
        const real w_eng = x[FB_X_ENG_OMEGA];
        const real w_prop = w_eng;  // gear ratio 1
        const v3 r_p = {prop_r[0], prop_r[1], prop_r[2]};
        const v3 v_p = v_wb_b + cross(w_eb_b, r_p);
        const real v_J = norm(v_p);
        const real J_adv = 2 * PI * v_J / (fmax(fabs(w_prop), FBL(1.0)) * prop_d);
        const real Mt = fabs(w_prop) * (prop_d / 2) * i_a_snd;
        const loc lj = range_locate(FBL(0.0), FBL(1.5), PR_NJ, J_adv, true);
        const loc lm = range_locate(FBL(0.0), FBL(1.5), PR_NM, Mt, true);
        lds_cptr c00 = PR + (lj.i + PR_NJ * lm.i) * NC;
        lds_cptr c10 = c00 + NC;
        lds_cptr c01 = c00 + PR_NJ * NC;
        lds_cptr c11 = c01 + NC;
        const real w00 = (1 - lj.w) * (1 - lm.w), w01 = (1 - lj.w) * lm.w, w10 = lj.w * (1 - lm.w), w11 = lj.w * lm.w;
        auto coef = [&](int cidx) { return (w00 * tab(c00, cidx) + w01 * tab(c01, cidx)) + (w10 * tab(c10, cidx) + w11 * tab(c11, cidx)); };
        const real C_Fx = coef(0), C_Mx = coef(1), C_Fz_a = coef(2), C_Mz_a = coef(3);
        real a_p = 0, b_p = 0;
        if (!(v_J < FBL(0.1))) {
            a_p = atan2m(v_p.z, v_p.x);
            b_p = atan2p(v_p.y, sqrt(v_p.x * v_p.x + v_p.z * v_p.z));
        }
        const real fr = w_prop / (2 * PI), fr2 = fr * fr;
        constexpr real d4 = prop_d * prop_d * prop_d * prop_d, d5 = d4 * prop_d;
        const real kF = rho * fr2 * d4, kM = rho * fr2 * d5;
        const v3 F_p = {kF * C_Fx, kF * (C_Fz_a * b_p), kF * (C_Fz_a * a_p)};
        const v3 tau_p = {kM * C_Mx, kM * (C_Mz_a * b_p), kM * (C_Mz_a * a_p)};  // CW: sense = +1
        const v3 tau_pb = tau_p + cross(r_p, F_p);
        F_b = F_b + F_p;
        tau_b = tau_b + tau_pb;
        h_rot = {prop_Jxx * w_prop, FBL(0.0), FBL(0.0)};
        PHASE_FENCE(9);

        // ---- engine ----
        real out_frc, out_idle;
        static_assert(FB_X_ENG_FRC == FB_X_ENG_IDLE + 1, "engine regulator rows are adjacent");
        const real kfrc = pi_ode(FBL(5.0), FBL(200.0), FBL(0.0), -FBL(1.0), FBL(1.0), -w_eng, x[FB_X_ENG_FRC], out_frc);
        const real ke2[2] = {pi_ode(FBL(4.0), FBL(2.0), FBL(0.0), -FBL(0.5), FBL(0.5), 1 - w_eng / w_idle, x[FB_X_ENG_IDLE], out_idle), kfrc};
        emit_rows<2>(emit, FB_X_ENG_IDLE, ke2);
        const real mu_ratio_idle = FBL(0.5) + out_idle;
        const real n_eng = w_eng / w_rated;
        // T_ISA(p) = T_std (p/p_std)^(-βR/g), δ = (p/p_std) (T_ISA/T_std)^-1/2 (piston.jl:38-41)
        // with log(p/p_std) = log(p_sl/p_std) + log(p/p_sl) from the atmosphere block: one exp, no log, no square root
        const real rt_arg = (FBL(0.5) * FBL(6.5e-3) * isa::R / isa::g_std) * (env.ln_p_sl + lnp_air);
        real rt_theta;   // (T_ISA/T_std)^1/2
        if constexpr (FASTM) {
            // In the troposphere p/p_sl = (T/T_sl)^(g/βR) and the exponent here is βR/2g, so (T_ISA/T_std)^1/2 =
            // (p_sl/p_std)^(βR/2g) (T/T_sl)^1/2 = k_rt sqrt(T): one multiply (sqrt T is at hand). Above 11 km, the general form;
            // a wave with no such lane skips it.
            const bool tropo = h_gp < FBL(11000.0);
            rt_theta = env.k_rt * (T_air * rs_T);
            if (__builtin_amdgcn_ballot_w64(!tropo) != 0) { const real e = exp_step(rt_arg); rt_theta = tropo ? rt_theta : e; }
        } else {
            rt_theta = exp(rt_arg);
        }
        const real T_ISA = isa::T_std * (rt_theta * rt_theta);
        const real delta = (p_air / isa::p_std) / rt_theta;
        const real throttle = in.get_throttle(), mixture = in.get_mixture();
        const loc l_n2 = range_locate(FBL(0.667), FBL(1.0), 2, n_eng, false);
        const real mu_wot = lerp2(PT + PT_MU_WOT_V, 2, l_n2, range_locate(FBL(0.441), FBL(1.0), 9, delta, false));
        const real mu = mu_wot * (mu_ratio_idle + throttle * (1 - mu_ratio_idle));
        const real k_f = rsqrt(rho * (1 / isa::rho_std));
        // Branch-free on purpose: the running-engine chain (five dependent table lookups) is evaluated for every
        // lane and the off / starting cases are selected at the end, so that the whole power-plant phase is one
        // basic block the scheduler can interleave (at one wave per SIMD, LDS latency is hidden only by ILP).
        // Every lookup clamps or extrapolates its index, so evaluating it for a stopped engine is harmless.
        // mixture_pos = (f_lean + mixture (f_rich - f_lean)) / (k_f f_rich) in auto mode, (mixture + 1) / 2 otherwise, and the
        // fuel-to-air ratio is k_f f_rich mixture_pos (piston.jl:352-366): in auto mode the two factors cancel
        const bool mix_auto = in.ui & FB_UI_MIXTURE_AUTO;
        const real f_run = mix_auto ? f_lean + mixture * (f_rich - f_lean) : k_f * (f_rich * (FBL(0.5) * (mixture + 1)));
        [[maybe_unused]] const real mixture_pos = mix_auto ? (f_lean + mixture * (f_rich - f_lean)) / (k_f * f_rich) : FBL(0.5) * (mixture + 1);   // (outputs only)
        // compute_π_ISA_pow (piston.jl:457-477)
        const loc l_n13 = grid_locate<13, SCALAR_KNOTS, AUX_N13>(PT + PT_PISTD_N_K, RPT + PT_PISTD_N_K, n_eng, true, true, gkp(LDS_PISTON + PT_PISTD_N_K), T.gk);
        const loc l_n5w = grid_locate<5, SCALAR_KNOTS>(PT + PT_PIWOT_N_K, RPT + PT_PIWOT_N_K, n_eng, true, true, gkp(LDS_PISTON + PT_PIWOT_N_K));
        const loc l_n5s = grid_locate<5, SCALAR_KNOTS>(PT + PT_SFC_N_K, RPT + PT_SFC_N_K, n_eng, false, false, gkp(LDS_PISTON + PT_SFC_N_K));
        const loc l_f = grid_locate<11, SCALAR_KNOTS, AUX_F11>(PT + PT_F_K, RPT + PT_F_K, f_run, true, true, gkp(LDS_PISTON + PT_F_K), T.gk);
        const real pi_ratio = lerp1(PT + PT_PI_RATIO_V, l_f), sfc_ratio = lerp1(PT + PT_SFC_RATIO_V, l_f);
        PHASE_FENCE(10);
        const real d_wot = lerp2(PT + PT_DELTA_WOT_V, 2, l_n2, range_locate(FBL(0.401), FBL(0.936), 9, mu, false));
        const real pi_std = lerp2(PT + PT_PISTD_V, 13, l_n13, grid_locate<3, SCALAR_KNOTS>(PT + PT_PISTD_MU_K, RPT + PT_PISTD_MU_K, mu, true, true, gkp(LDS_PISTON + PT_PISTD_MU_K)));
        const real pi_wot = lerp2(PT + PT_PIWOT_V, 5, l_n5w, grid_locate<3, SCALAR_KNOTS>(PT + PT_PIWOT_D_K, RPT + PT_PIWOT_D_K, d_wot, true, false, gkp(LDS_PISTON + PT_PIWOT_D_K)));
        real pi_isa = (fabs(d_wot - 1) < FBL(5e-3)) ? pi_std : pi_std + (pi_wot - pi_std) / (d_wot - 1) * (delta - 1);
        pi_isa = fmax(pi_isa, FBL(0.0));
        const real pi_pow = pi_isa * (rt_theta * (isa_sqrt_T_std * rs_T));   // pi_isa (T_ISA / T)^1/2
        const real pi_act = pi_pow * pi_ratio;
        const real P_run = P_rated * pi_act;
        const real tau_run = (w_eng > 0) ? P_run / w_eng : FBL(0.0);
        const real SFC_run = lerp2(PT + PT_SFC_POW_V, 5, l_n5s, grid_locate<8, SCALAR_KNOTS>(PT + PT_SFC_PI_K, RPT + PT_SFC_PI_K, pi_act, false, false, gkp(LDS_PISTON + PT_SFC_PI_K))) * sfc_ratio;
        const bool eng_off = eng_state == 0, eng_starting = eng_state == 1, eng_running = !(eng_off || eng_starting);
        const real MAP = eng_off ? p_air : mu * isa::p_std;
        const real f_ar = eng_running ? f_run : FBL(0.0);
        const real tau_shaft = eng_off ? out_frc * (FBL(0.01) * P_rated / w_rated) : (eng_starting ? tau_start : tau_run);
        const real P_shaft = eng_off ? FBL(0.0) : (eng_starting ? tau_start * w_eng : P_run);
        const real SFC = eng_running ? SFC_run : FBL(0.0);
        mdot = eng_running ? SFC_run * P_run : FBL(0.0);
        const real tau_load = tau_p.x;  // gear_ratio * τ_prop
        emit(FB_X_ENG_OMEGA, (tau_shaft + tau_load) / (J_eng + prop_Jxx));
        if (WITH_Y) {
            const int k = FB_Y_PWP;
            YP(k, MAP); YP(k + 1, f_ar); YP(k + 2, mdot); YP(k + 3, w_eng); YP(k + 4, tau_shaft); YP(k + 5, P_shaft); YP(k + 6, SFC);
            YP(k + 7, out_idle); YP(k + 8, out_frc);
            YP(k + 9, J_adv); YP(k + 10, Mt); YP3(k + 11, F_p); YP3(k + 14, tau_pb); YP3(k + 17, h_rot);
            if constexpr (SinkT::full) { YP(k + 20, rho * fabs(fr * fr2) * d5 * coef(4)); YP(k + 21, coef(5)); }
        }
    }

    emit(FB_X_FUEL, -mdot / (m_full - m_res));

    PHASE_FENCE(8);
    // ===== rigid-body dynamics at the CoM (dynamics.jl:443-525) =====
    {
        v3 d_e;
        const v3 w_ie_b = earth_rate_b(q_eb);
        const v3 g_c_c = gravity_com(q_eb, r_bc, n_e, h_e, R_N, R_E, i_RN, i_RE, st, d_e);
        const v3 tau_c = tau_b - cross(r_bc, F_b);
        auto Jmul = [&](v3 v) { return v3{Jxx * v.x + Jxy * v.y + Jxz * v.z, Jxy * v.x + Jyy * v.y + Jyz * v.z, Jxz * v.x + Jyz * v.y + Jzz * v.z}; };
        const v3 F_c = F_b;
        const v3 v_ec_c = v_eb_b + cross(w_eb_b, r_bc);
        const v3 w_ic_c = w_ie_b + w_eb_b;
        [[maybe_unused]] const v3 r_ec_e = r_eb_e + d_e;   // (outputs only)

        const v3 hc = Jmul(w_ic_c) + h_rot;
        const v3 rhs_w = tau_c - Jmul(cross(w_ie_b, w_eb_b)) - cross(w_ic_c, hc);
        // symmetric 3x3 solve by cofactors
        const real c11 = Jyy * Jzz - Jyz * Jyz, c12 = Jyz * Jxz - Jxy * Jzz, c13 = Jxy * Jyz - Jyy * Jxz;
        const real c22 = Jxx * Jzz - Jxz * Jxz, c23 = Jxy * Jxz - Jxx * Jyz, c33 = Jxx * Jyy - Jxy * Jxy;
        const real idet = 1 / (Jxx * c11 + Jxy * c12 + Jxz * c13);
        const v3 wd = {(c11 * rhs_w.x + c12 * rhs_w.y + c13 * rhs_w.z) * idet, (c12 * rhs_w.x + c22 * rhs_w.y + c23 * rhs_w.z) * idet,
                       (c13 * rhs_w.x + c23 * rhs_w.y + c33 * rhs_w.z) * idet};
        const v3 vd_c = iM * F_c + g_c_c - cross(w_eb_b + FBL(2.0) * w_ie_b, v_ec_c);
        const v3 vd_b = vd_c - cross(wd, r_bc);
        static_assert(FB_X_V_EB_B == FB_X_OMEGA_EB_B + 3, "the six dynamics rows are adjacent");
        const real kd6[6] = {wd.x, wd.y, wd.z, vd_b.x, vd_b.y, vd_b.z};
        emit_rows<6>(emit, FB_X_OMEGA_EB_B, kd6);
        if (WITH_Y) {
            const int k = FB_Y_DYN;
            YP(k, M); YP3(k + 1, r_bc);
            YP(k + 4, J[0]); YP(k + 5, J[3]); YP(k + 6, J[4]); YP(k + 7, J[3]); YP(k + 8, J[1]); YP(k + 9, J[5]); YP(k + 10, J[4]); YP(k + 11, J[5]); YP(k + 12, J[2]);
            YP3(k + 13, F_b); YP3(k + 16, tau_b); YP3(k + 19, wd); YP3(k + 22, vd_b);
            const v3 r_eb_b = qrot_inv(q_eb, r_eb_e), r_ec_c = qrot_inv(q_eb, r_ec_e);
            YP3(k + 25, vd_b + cross(w_eb_b, v_eb_b));
            YP3(k + 28, vd_b + cross(w_eb_b + FBL(2.0) * w_ie_b, v_eb_b) + cross(w_ie_b, cross(w_ie_b, r_eb_b)));
            const v3 a_ic = vd_c + cross(w_eb_b + FBL(2.0) * w_ie_b, v_ec_c) + cross(w_ie_b, cross(w_ie_b, r_ec_c));
            const v3 gam = g_c_c + cross(w_ie_b, cross(w_ie_b, r_ec_c));
            YP3(k + 31, a_ic - gam); YP3(k + 34, wd - cross(w_eb_b, w_ie_b)); YP3(k + 37, g_c_c);
        }
    }
    PHASE_FENCE(20);
    return st;
}

// f_step!(world): kinematics renormalisation, stall hysteresis, contact-regulator reset, crash checks,
// engine state machine (aircraftbase.jl:172-181; kinematics.jl:226-229,114-118; c172.jl:375-384,715-724;
// landinggear.jl:331-347,479-483; piston.jl:428-453). Returns true when x or s changed.
template <int KIN, class In, int NXT>
FBD bool f_step(real (&x)[NXT], int& stall, int& eng_state, const In& in, const StepAux& aux, int32_t& st) {
    bool mod = false;
    // normalize_block!(x, ε = 1e-8) (kinematics.jl:114-118) on q_wb, q_ew (WA :226-229) or q_eb, n_e (ECEF :317-320); NED: nothing
    auto renorm = [&](int k0, int len) {
        real n2 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < len) n2 += x[k0 + k] * x[k0 + k];
        const real nr = sqrt(n2);
        if (fabs(nr - FBL(1.0)) > FBL(1e-8)) {
#pragma unroll
            for (int k = 0; k < 4; k++) if (k < len) x[k0 + k] /= nr;
            mod = true;
        }
    };
    if constexpr (KIN == FB_KIN_WA) { renorm(FB_X_Q_WB, 4); renorm(FB_X_Q_EW, 4); }
    else if constexpr (KIN == FB_KIN_ECEF) { renorm(FB_X_Q_WB, 4); renorm(FB_X_Q_WB + 4, 3); }
    const int stall0 = stall, eng0 = eng_state;
    if (aux.alpha > c172::alpha_stall_hi) stall = 1;
    else if (aux.alpha < c172::alpha_stall_lo) stall = 0;
    // landing gear, unit by unit (c172.jl:485; landinggear.jl:539-548): the strut's crash check THROWS, and what follows it in the
    // reference's order — this unit's regulator reset, the later units, the engine's state machine — does not run (FC/sim.jl:561-570)
    bool crashed = false;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        if (crashed) continue;
        if (aux.crash & (1 << g)) { crashed = true; continue; }
        if (!(aux.wow & (1 << g))) {
            if (x[FB_X_LDG_FRC + 2 * g] != FBL(0.0) || x[FB_X_LDG_FRC + 2 * g + 1] != FBL(0.0)) mod = true;
            x[FB_X_LDG_FRC + 2 * g] = FBL(0.0);
            x[FB_X_LDG_FRC + 2 * g + 1] = FBL(0.0);
        }
    }
    if (crashed) { st |= FB_ST_GROUND_CRASH; return mod || stall != stall0; }
    const real w = x[FB_X_ENG_OMEGA];
    const bool fuel = aux.m_avail > 0;
    const bool start = in.ui & FB_UI_ENG_START, stop = in.ui & FB_UI_ENG_STOP;
    if (eng_state == 0) {
        if (start) eng_state = 1;
    } else if (eng_state == 1) {
        if (!start) eng_state = 0;
        if (w > c172::w_idle && fuel) eng_state = 2;
    } else {
        if (stop || w < c172::w_stall || !fuel) eng_state = 0;
    }
    return mod || stall != stall0 || eng_state != eng0;
}

}  // namespace FB_NS
