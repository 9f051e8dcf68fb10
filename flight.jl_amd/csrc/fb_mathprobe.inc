// fb_mathprobe.inc — the device math primitives of c172_device_impl.inc, one call per element, for the accuracy tests
// (include/flightbatch.h: fb_math_probe; tests/test_gpu_math_primitives.py; docs/design/k_step_air.md, "Math primitives, measured").
// Included by fb_capi.hip after fb_lss.inc (DevBlocks). The kernel lives in the shipped library on purpose: the primitives are then
// compiled with the shipped flags (-fapprox-func, -freciprocal-math, the 2.5-ulp fp32 divide and sqrt) and pass the same spill gate
// as the stepping kernels, so what is measured is what flies. It calls fbd:: / fbf:: exactly as they do: the default constant
// provider KLit, and atan2_tab's table staged in LDS by the expression of stage_tables (c172_kernels.hpp).
// Every thread reads and writes element i < n of its own arrays only; the one index that comes from the data (FB_MP_ATAN_TABLE) is clamped.

struct MathProbeArgs {
    int32_t op;
    int64_t n;
    const double *a, *b;   // b: null for a unary op
    double *o0, *o1;       // o1: null for an op with one output
};

__global__ __launch_bounds__(256) void k_math_probe(MathProbeArgs p) {
    __shared__ double tab_l[fbd::ATAN_N];
    for (int k = threadIdx.x; k < fbd::ATAN_N; k += blockDim.x) tab_l[k] = atan(k * (1.0 / 32));   // atan2_tab()'s table
    __syncthreads();
    const fbd::lds_cptr tab = (fbd::lds_cptr)tab_l;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const double a = p.a[i], b = p.b ? p.b[i] : 0.0;
    const float af = (float)a, bf = (float)b;   // the fp32 ops: the caller passes values that are floats already
    double r0 = 0.0, r1 = 0.0;
    switch (p.op) {   // (wave-uniform)
    case FB_MP_SQRT: r0 = fbd::sqrt(a); break;
    case FB_MP_RSQRT: r0 = fbd::rsqrt(a); break;
    case FB_MP_DIV: r0 = a / b; break;
    case FB_MP_RCP: r0 = 1 / a; break;
    case FB_MP_HALF_ANGLE: fbd::half_angle_cs(a, b, r0, r1); break;
    case FB_MP_ATAN2_TAB: r0 = fbd::atan2_step(a, b, tab); break;
    case FB_MP_ATAN2_TAB_XPOS: r0 = fbd::atan2_step<true>(a, b, tab); break;
    case FB_MP_LOG_NEAR1: r0 = fbd::log_near1(a); break;
    case FB_MP_SINCOS_STEP: fbd::sincos_step(a, r0, r1); break;
    case FB_MP_ISA_FAST:
    case FB_MP_ISA: {
        double T, pr, lnp;
        int32_t st = 0;
        if (p.op == FB_MP_ISA_FAST) fbd::isa_data<true>(a, b, 1.0, T, pr, lnp, st); else fbd::isa_data<false>(a, b, 1.0, T, pr, lnp, st);
        p.o0[i] = T; p.o0[p.n + i] = pr; p.o0[2 * p.n + i] = lnp;
        p.o1[i] = (double)st;
        return;
    }
    case FB_MP_ATAN_TABLE: r0 = tab[min(max((int)a, 0), fbd::ATAN_N - 1)]; break;
    case FB_MP_LIB_EXP: r0 = fbd::exp_step(a); break;    // (fp64: the library's exp / log)
    case FB_MP_LIB_LOG: r0 = fbd::log_step(a); break;
    case FB_MP_LIB_SINCOS: fb_sincos(a, &r0, &r1); break;
    case FB_MP_LIB_ATAN2: r0 = atan2(a, b); break;
    case FB_MP_F32_ATAN2_FAST: r0 = fbf::atan2_step(af, bf, nullptr); break;
    case FB_MP_F32_ATAN2_FAST_XPOS: r0 = fbf::atan2_step<true>(af, bf, nullptr); break;
    case FB_MP_F32_EXP_STEP: r0 = fbf::exp_step(af); break;
    case FB_MP_F32_LOG_STEP: r0 = fbf::log_step(af); break;
    case FB_MP_F32_SQRT: r0 = fbf::sqrt(af); break;
    case FB_MP_F32_RSQRT: r0 = fbf::rsqrt(af); break;
    case FB_MP_F32_DIV: r0 = af / bf; break;
    default: break;   // (refused on the host)
    }
    p.o0[i] = r0;
    if (p.o1) p.o1[i] = r1;
}

extern "C" {

int32_t fb_math_probe(int32_t op, int64_t n, const double* a, const double* b, double* out0, double* out1) {
    static const char* verb = "fb_math_probe";
    const bool f64 = op >= FB_MP_SQRT && op < FB_MP_F64_END, f32 = op >= FB_MP_F32_ATAN2_FAST && op < FB_MP_F32_END;
    if (!f64 && !f32) return fail("%s: unknown op %d (FB_MP_*)", verb, op);
    const bool isa = op == FB_MP_ISA_FAST || op == FB_MP_ISA;
    const bool binary = op == FB_MP_DIV || op == FB_MP_HALF_ANGLE || op == FB_MP_ATAN2_TAB || op == FB_MP_ATAN2_TAB_XPOS || isa ||
                        op == FB_MP_LIB_ATAN2 || op == FB_MP_F32_ATAN2_FAST || op == FB_MP_F32_ATAN2_FAST_XPOS || op == FB_MP_F32_DIV;
    const bool two = op == FB_MP_HALF_ANGLE || op == FB_MP_SINCOS_STEP || op == FB_MP_LIB_SINCOS || isa;
    if (n < 1 || n > FB_MP_N_MAX) return fail("%s: n = %lld, the call takes 1 <= n <= %d (FB_MP_N_MAX)", verb, (long long)n, (int)FB_MP_N_MAX);
    if (!a || !out0) return fail("%s: null a or out0", verb);
    if (binary && !b) return fail("%s: op %d takes two arguments and b is null", verb, op);
    if (two && !out1) return fail("%s: op %d has two outputs and out1 is null", verb, op);
    const size_t cnt = (size_t)n, n0 = isa ? 3 * cnt : cnt;
    DevBlocks blocks;
    double* d = nullptr;
    if (int32_t rc = blocks.alloc(&d, 3 * cnt + n0)) return rc;   // one block: a | b | out1 | out0
    MathProbeArgs p = {op, n, d, binary ? d + cnt : nullptr, d + 3 * cnt, two ? d + 2 * cnt : nullptr};
    HIPCHK(hipMemcpy(d, a, sizeof(double) * cnt, hipMemcpyHostToDevice));
    if (binary) HIPCHK(hipMemcpy(d + cnt, b, sizeof(double) * cnt, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_math_probe, grid_for(n, 256), dim3(256), 0, nullptr, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out0, p.o0, sizeof(double) * n0, hipMemcpyDeviceToHost));   // (synchronises with the kernel on the null stream)
    if (two) HIPCHK(hipMemcpy(out1, p.o1, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
