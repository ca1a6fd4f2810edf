// pt_denoise_dev.h -- what the filter's translation units (pt_denoise.hip, pt_temporal.hip, pt_records.hip) share on the device, and the grid
// all their per-pixel kernels run on.  f32 under -ffp-contract=off: the order of every operation here is contract (the records' v and the
// temporal depth tolerance are these expressions' bits)
#pragma once
#include "pt_device.h"

namespace prt {

PT_DEV float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
PT_DEV bool dn_finite3(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }

// the luminance variance of pixel id's mean from the stats plane {l, s2} and the path count of the state; fewer than two paths: 0
PT_DEV float dn_stats_var(const uint4* __restrict__ q4, const float2* __restrict__ adapt, size_t id) {
    float v = 0.0f;
    const unsigned n = q4[id].x;
    if (n >= 2u) {
        const float2 a = adapt[id];
        const float m = a.x / (float)n;
        v = fmaxf((a.y - a.x * m) / ((float)n * (float)(n - 1u)), 0.0f);
    }
    return v;
}

// one-sided / central difference of z at p towards (x + sx, y + sy) and (x - sx, y - sy); a neighbour outside the frame or without
// coverage drops out (both out: 0)
PT_DEV float dn_grad1(const float4* __restrict__ gd, int x, int y, int sx, int sy, int W, int H, float zp) {
    const int xa = x + sx, ya = y + sy, xb = x - sx, yb = y - sy;
    const bool a_in = xa < W && ya < H, b_in = xb >= 0 && yb >= 0;
    bool ha = false, hb = false;
    float za = 0.0f, zb = 0.0f;
    if (a_in) { const size_t q = (size_t)ya * W + xa; ha = gd[2 * q].w > 0.0f; za = gd[2 * q + 1].w; }
    if (b_in) { const size_t q = (size_t)yb * W + xb; hb = gd[2 * q].w > 0.0f; zb = gd[2 * q + 1].w; }
    if (ha && hb) return 0.5f * fabsf(za - zb);
    if (ha) return fabsf(za - zp);
    if (hb) return fabsf(zp - zb);
    return 0.0f;
}

// 16x16 workgroups, one lane per pixel: the kernels compute x = blockIdx.x * 16 + threadIdx.x, y likewise, and leave outside W x H
inline dim3 dn_block() { return dim3(16, 16); }
inline dim3 dn_grid(int W, int H) { return dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)); }

}  // namespace prt
