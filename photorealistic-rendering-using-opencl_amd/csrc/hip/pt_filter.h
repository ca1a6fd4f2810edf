// pt_filter.h -- pixel reconstruction filters of the primary rays (prt_set_pixel_filter, include/prt.h has the contract).  No counterpart in the
// reference (its camera has no jitter).  Filter importance sampling (Ernst et al. 2006): path k of a pixel starts through the pixel centre
// plus an offset drawn from the filter, every sample with weight 1.  Host and device compile this same text: the host entry point
// prt_pixel_filter_offsets, the PT_MATS_FILTER instances of render_kernel (lane_front), the filtered guide kernel and the self-test (fn 12).
#pragma once
#include <hip/hip_runtime.h>

#include "prt.h"

namespace prt {
namespace dev {

#define PT_FILTER_TAB 256                      // segments of the inverse-CDF table of the Gaussian and Blackman-Harris kinds (257 entries)

__host__ __device__ __forceinline__ unsigned filter_lowbias32(unsigned v) {
    v ^= v >> 16; v *= 0x7FEB352Du; v ^= v >> 15; v *= 0x846CA68Bu; v ^= v >> 16;
    return v;
}

// the warp w of prt.h: u in [0, 1) -> an offset in [-r, r] distributed as the filter's marginal.  tab: the table kinds' T[0 .. 256]
__host__ __device__ __forceinline__ float filter_warp(unsigned kind, float r, const float* tab, float u) {
    if (kind == PRT_FILTER_BOX) return (u - 0.5f) * (2.0f * r);
    if (kind == PRT_FILTER_TENT) return u < 0.5f ? r * (__builtin_sqrtf(2.0f * u) - 1.0f) : r * (1.0f - __builtin_sqrtf(2.0f - 2.0f * u));
    float t = u * (float)PT_FILTER_TAB;
    int j = (int)t;
    if (j > PT_FILTER_TAB - 1) j = PT_FILTER_TAB - 1;  // (u < 1 on every path of the library: a guard for the table's bounds)
    t -= (float)j;
    return tab[j] + t * (tab[j + 1] - tab[j]);
}

// the offset (dx, dy) of path k (0-based, since the last reset) of global pixel (gx, gy): the R2 sequence in 0.32 fixed point, rotated per
// pixel by a hash of its coordinates, then warped.  No draw from the path's RNG stream
__host__ __device__ __forceinline__ void filter_offset(unsigned kind, float r, const float* tab, unsigned gx, unsigned gy, unsigned k,
                                                       float& dx, float& dy) {
    const unsigned s = gy * 0x9E3779B9u + gx;
    const unsigned ux = k * 3242174889u + filter_lowbias32(s);
    const unsigned uy = k * 2447445414u + filter_lowbias32(s ^ 0x68E31DA4u);
    dx = filter_warp(kind, r, tab, (float)(ux >> 8) * 5.9604644775390625e-08f);      // (exact: 24 bits times 2^-24)
    dy = filter_warp(kind, r, tab, (float)(uy >> 8) * 5.9604644775390625e-08f);
}

}  // namespace dev
}  // namespace prt
