// lss_group.hpp — what the kernels of the LinearizedSS family (lss, lqr, pid, poles, timeresp, connect, surgery _kernels.hpp) share on the device
// (docs/design/linearize.md, "What the family shares"). Every one of them gives a system, or a (system, something) pair, to a group of P
// lanes of one wave: 64 / P groups per wave, a group never straddles a wave, lane r of a group owns row r.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>

namespace fbg {

constexpr int WAVE = 64;

// a panel belongs to one wave, whose LDS operations are performed in issue order: only the compiler is kept from moving them (no s_barrier)
__device__ inline void panel_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__host__ __device__ inline bool is_fin(double v) { return fabs(v) <= DBL_MAX; }   // false for NaN

struct Pivot { int p; double m; bool found; };   // of an elimination step: the lane that holds it, its magnitude, whether it is usable

// this lane's group of P lanes: lane index, first lane of the group in the wave, and the group-wide operations
template <int P>
struct Lanes {
    int r, base;
    __device__ Lanes() : r(threadIdx.x % P), base((threadIdx.x / P) * P) {}
    __device__ double gmax(double v) const {
#pragma unroll
        for (int o = P / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, P));
        return v;
    }
    __device__ unsigned mask(bool b) const { return (unsigned)((__ballot(b) >> base) & (P == 32 ? 0xffffffffull : ((1ull << P) - 1))); }
    __device__ bool any(bool b) const { return mask(b) != 0; }
    // the family's pivot rule: the group-wide maximum m of v over the rows not yet `used`, then the lowest lane that holds it; not found
    // (p = k, the arithmetic goes on) when no row is left or m is zero or not finite
    __device__ __forceinline__ Pivot pivot(bool used, double v, int k) const {
        const double m = gmax(v);
        const unsigned cand = mask(!used && v == m);
        return {cand ? __builtin_ctz(cand) : k, m, cand != 0 && m > 0.0 && is_fin(m)};
    }
};

template <int P>
__device__ inline double gsum(double v) {
#pragma unroll
    for (int o = P / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, P);
    return v;
}
// the minimum / maximum over the whole wave of a value that is uniform within each group of P lanes, as a scalar
template <int P>
__device__ inline int wave_min(int v) {
#pragma unroll
    for (int o = P; o < WAVE; o <<= 1) v = min(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
template <int P>
__device__ inline int wave_max(int v) {
#pragma unroll
    for (int o = P; o < WAVE; o <<= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}

// Exchange of the G stage values dz of a group, one per lane (docs/design/linearize.md, "Model(lss) on the device"): XCH = 0, an LDS panel
// of one double per lane, read back as G / 2 16-byte broadcasts; XCH = 1, G cross-lane reads (two ds_bpermute_b32 each) and no LDS
template <int G, int XCH>
struct Exchange {
    double* row;       // XCH == 0: this group's G doubles of the panel
    double* mine;
    __device__ Exchange(double* panel) : row(panel + (threadIdx.x / G) * G), mine(panel + threadIdx.x) {}
    // acc + sum_c a[c] dz_c, c ascending
    __device__ double dot(const double (&a)[G], double dz, double acc) const {
        if constexpr (XCH == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            *mine = dz;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double2* p = reinterpret_cast<const double2*>(row);
#pragma unroll
            for (int c = 0; c < G; c += 2) {
                const double2 v = p[c / 2];
                acc = fma(a[c], v.x, acc);
                acc = fma(a[c + 1], v.y, acc);
            }
        } else {
#pragma unroll
            for (int c = 0; c < G; c++) acc = fma(a[c], __shfl(dz, c, G), acc);
        }
        return acc;
    }
};

// stages 2 .. 4 of an RK4 step whose first stage is k1, and the step; a lane without a state publishes 0. Explicit fma: loops round alike.
template <int P>
__device__ inline double rk4_finish(const Exchange<P, 0>& ex, const double (&row)[P], double c0, bool state, double x, double k1,
                                    double dt, double hdt, double dt6) {
    const double k2 = ex.dot(row, state ? fma(hdt, k1, x) : 0.0, c0);
    const double k3 = ex.dot(row, state ? fma(hdt, k2, x) : 0.0, c0);
    const double k4 = ex.dot(row, state ? fma(dt, k3, x) : 0.0, c0);
    return state ? fma(dt6, 2 * (k2 + k3) + (k1 + k4), x) : 0.0;
}

// The handle's copy of the model (written by fbl::k_lss_gather only), for n systems with group size G (4, 8, 16 or 32, the smallest >= nx),
// slot = i G + r and S = n G:
//   ab [(G + nu) x S]   column c of row r of [A | B] at ab[c S + slot] (A's columns zero-padded to G, B at column G + k): the loads of a
//                       group's lanes r are coalesced. Rows r >= nx and columns nx <= c < G are exact zeros.
//   xs [2 x S]          xdot0_r, x0_r (zeros for r >= nx)
//   u0 [nu x n], y0 [ny x n]
//   cd [(nx + nu) x n x ny]   element (j, c) of [C | D] at cd[(c n + i) ny + j] (D at column nx + k): the lanes of a group read
//                       consecutive rows j
// The ONE statement of where an element lies: two index functions for every reader, the writer and the host's un-padding, the pointer named
// where it is read (a kernel's code depends on where its argument loads stand). Column c of [A | B] (B's k: c = G + k) of the system's row 0,
// slot0 = i G, row r being r further; element (j, c) of [C | D] (D's k: c = nx + k). Inlined before anything is optimised: the same code.
__host__ __device__ __forceinline__ int64_t ab_index(int64_t S, int64_t slot0, int64_t c) { return c * S + slot0; }
__host__ __device__ __forceinline__ int64_t cd_index(int64_t n, int64_t i, int ny, int j, int c) { return ((int64_t)c * n + i) * ny + j; }

// A staged model, the layout fb_linearize writes (include/flightbatch.h) and every verb that makes or returns a model stages its result in,
// for n systems: xdot0 | x0 [nx x n] | u0 [nu x n] | y0 [ny x n] | AB | CD, a vector's row r of system i at [r n + i], and element (r, c)
// of a matrix block of `rows` rows at [(r + rows c) n + i]: AB = [A | B] with rows = nx (B's k: c = nx + k), CD = [C | D] with rows = ny;
// the blocks a verb returns alone (X, K, U, K_fwd) are laid out the same way. The ONE statement of that index, as above.
__host__ __device__ __forceinline__ int64_t staged_index(int64_t n, int64_t i, int rows, int64_t r, int64_t c) { return (r + (int64_t)rows * c) * n + i; }

// whether every entry of system i's [A | B] and [C | D] in a handle's copy is finite: lane r of a group of P looks at row r of [A | B] and
// at rows r, r + P, ... of [C | D]
template <int P>
__device__ inline bool model_finite(const double* ab, const double* cd, int nx, int nu, int ny, int G, int64_t n, int64_t i, int r) {
    bool fin = true;
    const int64_t S = n * G, slot0 = i * G;
    if (r < nx) {
        for (int c = 0; c < nx; c++) fin = fin && is_fin(ab[ab_index(S, slot0, c) + r]);
        for (int c = 0; c < nu; c++) fin = fin && is_fin(ab[ab_index(S, slot0, G + c) + r]);
    }
    for (int c = 0; c < nx + nu; c++)
        for (int j = r; j < ny; j += P) fin = fin && is_fin(cd[cd_index(n, i, ny, j, c)]);
    return fin;
}

// The family's solve of [E | rhs] (k_transform, k_steady; k_connect mirrors it by hand; numpy restatement: tests/surgery_prototype.py, solve): Gauss-Jordan
// elimination with the pivot rule above on the rows of a group, which stay with their lanes. Lane r < steps (`live`) holds row r: e, the NE
// columns that are eliminated, and rhs, NR right-hand columns (NE and NR even). Every step is a compile-time k, the steps k >= steps behind
// a wave-uniform branch. The pivot lane scales its row and puts it at the group's `prow` [NE + NR], the other live lanes subtract it as
// 16-byte broadcasts; the column of a step is not kept (it would be a unit vector). The lane that was the pivot of step k ends with row k
// of the solution and puts it at row k of `sol` [. x LD], where every lane of the group may read it once gj_solve has returned.
// ok: every step found a pivot; pmin, pmax: the smallest and largest pivot magnitude. The arithmetic goes on past a missing pivot.
// The row goes in by value (as Pivot comes out): by reference the same arithmetic takes up to 32 registers more (profiles/lss_solve_refactor.txt).
template <int NE, int NR> struct Row { double e[NE], rhs[NR]; };
struct Solve { bool ok; double pmin, pmax; };
template <int P, int LD, int NE, int NR>
__device__ __forceinline__ Solve gj_solve(const Lanes<P>& g, Row<NE, NR> w, double* prow, double* sol, bool live, int steps) {
    bool used = !live;
    int myk = 0;
    Solve s = {true, DBL_MAX, 0.0};
#pragma unroll
    for (int k = 0; k < NE; k++) {
        if (k < steps) {
            const Pivot pv = g.pivot(used, used ? -1.0 : fabs(w.e[k]), k);
            s.ok = s.ok && pv.found;
            s.pmin = fmin(s.pmin, pv.m);
            s.pmax = fmax(s.pmax, pv.m);
            panel_sync();
            if (g.r == pv.p) {
                const double ip = 1.0 / w.e[k];
#pragma unroll
                for (int j = k + 1; j < NE; j++) { w.e[j] *= ip; prow[j] = w.e[j]; }
#pragma unroll
                for (int j = 0; j < NR; j++) { w.rhs[j] *= ip; prow[NE + j] = w.rhs[j]; }
                used = true; myk = k;
            }
            panel_sync();
            if (live && g.r != pv.p) {
                const double f = w.e[k];
#pragma unroll
                for (int j = k + 1; j < NE; j++) w.e[j] = fma(-f, prow[j], w.e[j]);
                const double2* row = reinterpret_cast<const double2*>(prow + NE);
#pragma unroll
                for (int j = 0; j < NR; j += 2) {
                    const double2 v = row[j / 2];
                    w.rhs[j] = fma(-f, v.x, w.rhs[j]);
                    w.rhs[j + 1] = fma(-f, v.y, w.rhs[j + 1]);
                }
            }
        }
    }
    panel_sync();
    if (live) {
#pragma unroll
        for (int j = 0; j < NR; j++) sol[myk * LD + j] = w.rhs[j];
    }
    panel_sync();
    return s;
}

// what a solve says of its system: a non-finite input is reported first, then the pivots; rpiv is the smallest pivot magnitude over the
// largest. A system with a status stores NaN.
struct Verdict { int32_t status; double rpiv; };
template <int P>
__device__ inline Verdict verdict(const Lanes<P>& g, bool fin, const Solve& s, int32_t not_finite, int32_t singular) {
    if (g.any(!fin)) return {not_finite, __builtin_nan("")};
    if (g.any(!s.ok)) return {singular, 0.0};
    return {0, s.pmin / s.pmax};
}

}  // namespace fbg
