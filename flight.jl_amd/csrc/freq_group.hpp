// freq_group.hpp — what the margins kernels of both time domains share on the device: fbn::k_lss_margins (margins_kernels.hpp) and
// fbw::k_lss_dmargins (dfreq_kernels.hpp), docs/design/linearize.md, "What the family shares". The complex elimination and the margins
// body are NOT here: written as one function they do not keep the kernels' bits (profiles/freq_family_refactor.txt), so each kernel keeps
// its own text.
#pragma once
#include "lss_group.hpp"

namespace fbg {

__device__ __forceinline__ double mag2(double lr, double li) { return fma(lr, lr, li * li); }
// whether the gain margin g = -Re L* is closer to 1 than h is, in either direction: max(g, 1 / g) < max(h, 1 / h) without dividing
__device__ __forceinline__ bool closer_to_one(double g, double h) {
    if (g >= 1.0 && h >= 1.0) return g < h;
    if (g < 1.0 && h < 1.0) return g > h;
    const double gh = g * h;
    return g >= 1.0 ? gh < 1.0 : gh > 1.0;
}

}  // namespace fbg
