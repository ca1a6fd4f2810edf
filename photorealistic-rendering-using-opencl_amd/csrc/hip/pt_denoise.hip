// pt_denoise.hip -- feature buffers and the edge-aware a-trous filter (prt_render_guides, prt_denoise; include/prt.h has the contract).
// A translation unit of its own: no code object of the render kernels changes with it.
//
//   guide_kernel<SDF>   K guide samples per pixel (pt_guides.h), one lane per pixel, 8x8 tiles per 64-lane wave
//   guide_motion_kernel<SDF>, filtered_guides_motion_kernel   the same, and the motion plane (pt_motion.h; prt.h prt_set_motion)
//   guide_prim_motion_kernel<SDF, TRI>, filtered_guides_prim_motion_kernel<TRI>   the motion plane with a primitive snapshot pending (pt_prims.h;
//                       prt.h prt_update_primitives), with (TRI) or without the triangle term
//   dn_var_kernel       {rgb, v} per pixel: the framebuffer colour and the luminance variance of its mean (stats plane or 5x5 moments)
//   dn_gauss_kernel     3x3 Gaussian of v (one per pass)
//   dn_atrous_kernel    one a-trous pass: 5x5 taps at step 2^i, weights from normal, depth, albedo and luminance; ping-pongs {rgb, v}
//
// The filter kernels run 16x16 workgroups over the frame and read straight from global memory: at 1080p the working set (guides,
// ping-pong buffers, framebuffer) stays in the L2 / Infinity Cache, a tap costs three 16-byte loads.
#include "pt_guides.h"
#include "pt_launch.h"
#include "pt_motion.h"
#include "pt_prims.h"

namespace prt {
using namespace dev;

// ---- guides --------------------------------------------------------------------------------------------------------------------------
// FILTER: the sample offsets warped by the context's pixel filter (prt.h prt_set_pixel_filter; filtered_guides_kernel)
// MOTION: also the motion plane {D, m} of the pixel, from the triangle records before the update(s) (tri_prev: an argument of its own, DevScene
// is the render kernels' kernarg block) and sc.tri_geom; the eight guide floats are the other instances' bit for bit
// PRIM: the plane also carries the first hits on spheres, SDF primitives and quads, from the tables before the update(s) (prims) and
// sc.spheres / sc.sdfs / sc.quads: the records of the lane's own hit, read per lane.  MOTION then says whether a triangle snapshot is pending
// too: without one the triangle term is not compiled in
template <bool SDF, bool FILTER, bool MOTION, bool PRIM = false>
PT_DEV void guide_pixel(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* __restrict__ out,
                        const TriGeom* __restrict__ tri_prev, float4* __restrict__ motion, const PrimPrev prims = PrimPrev{nullptr, nullptr, nullptr}) {
    const int tiles_x = (fa.width + 7) / 8;
    const int lane = threadIdx.x & 63;
    const int lx = (int)(blockIdx.x % (unsigned)tiles_x) * 8 + (lane & 7);
    const int ly = (int)(blockIdx.x / (unsigned)tiles_x) * 8 + (lane >> 3);
    extern __shared__ unsigned lds_stack[];                     // sc.stack_levels x 64, sized by the launch
    TravStack stk;
    stk.lds = lds_stack + threadIdx.x; stk.stride = 64;
    if (lx >= fa.width || ly >= fa.rows) return;
    const int gx = lx;
    const int gy = fa.row0 + (ly / fa.block_rows * fa.n_parts + fa.part) * fa.block_rows + ly % fa.block_rows;
    f3 albedo = splat(0.0f), nsum = splat(0.0f);
    float zsum = 0.0f;
    unsigned hits = 0;
    MotionSum msum = motion_sum_begin();
    for (unsigned s = 0; s < samples; ++s) {
        float fx, fy;
        guide_offsets(s, fx, fy);
        Ray ray;
        if constexpr (FILTER)
            ray = guide_cam_ray_at(gx, gy, fa.width, fa.full_height, cam, filter_warp(fa.filter_kind, fa.filter_r, fa.filter_tab, fx),
                                   filter_warp(fa.filter_kind, fa.filter_r, fa.filter_tab, fy), guide_frac(fx + 0.25f), guide_frac(fy + 0.75f));
        else
            ray = guide_cam_ray(gx, gy, fa.width, fa.full_height, cam, fx, fy, guide_frac(fx + 0.25f), guide_frac(fy + 0.75f));
        const GuideSample g = guide_sample<SDF>(sc, ray, stk);
        albedo = albedo + g.albedo;
        if (g.hit) {
            ++hits;
            zsum = zsum + g.depth;
            if (dot(g.normal, g.normal) == dot(g.normal, g.normal)) nsum = nsum + g.normal;     // (a degenerate mesh normal is NaN: left out)
            if constexpr (MOTION)
                if (g.direct_triangle) motion_sum_add(msum, motion_displacement(tri_prev, sc.tri_geom, g.slot, g.u, g.v));
            if constexpr (PRIM)
                if (g.direct_prim)
                    motion_sum_add(msum, prims_displacement(prims, sc.spheres, sc.sdfs, sc.quads, sc.n_spheres, SDF ? sc.n_sdfs : 0u, sc.quad_mesh_base,
                                                            (unsigned)g.mid, g.pos.x, g.pos.y, g.pos.z));
        }
    }
    const float inv_k = 1.0f / (float)samples;
    const float len2 = dot(nsum, nsum);
    const f3 n = len2 > 0.0f ? nsum * (1.0f / sqrtf(len2)) : splat(0.0f);
    const size_t id = (size_t)ly * (size_t)fa.width + (size_t)lx;
    out[2 * id] = make_float4(albedo.x * inv_k, albedo.y * inv_k, albedo.z * inv_k, (float)hits * inv_k);
    out[2 * id + 1] = make_float4(n.x, n.y, n.z, hits ? zsum / (float)hits : 0.0f);
    if constexpr (MOTION || PRIM) {
        const MotionQuad m = motion_pixel(msum, hits, samples);
        motion[id] = make_float4(m.x, m.y, m.z, m.w);
    }
}
template <bool SDF>
__global__ __launch_bounds__(64) void guide_kernel(const DevScene sc, const DevCamera cam, const FrameArgs fa, unsigned samples,
                                                   float4* __restrict__ out) {
    guide_pixel<SDF, false, false>(sc, cam, fa, samples, out, nullptr, nullptr);
}
// under a pixel filter (no SDF build: prt_set_pixel_filter refuses SDF scenes)
__global__ __launch_bounds__(64) void filtered_guides_kernel(const DevScene sc, const DevCamera cam, const FrameArgs fa, unsigned samples,
                                                          float4* __restrict__ out) {
    guide_pixel<false, true, false>(sc, cam, fa, samples, out, nullptr, nullptr);
}
// the motion instances: plain, SDF, pixel filter
template <bool SDF>
__global__ __launch_bounds__(64) void guide_motion_kernel(const DevScene sc, const DevCamera cam, const FrameArgs fa, unsigned samples,
                                                          float4* __restrict__ out, const TriGeom* __restrict__ tri_prev,
                                                          float4* __restrict__ motion) {
    guide_pixel<SDF, false, true>(sc, cam, fa, samples, out, tri_prev, motion);
}
__global__ __launch_bounds__(64) void filtered_guides_motion_kernel(const DevScene sc, const DevCamera cam, const FrameArgs fa, unsigned samples,
                                                                    float4* __restrict__ out, const TriGeom* __restrict__ tri_prev,
                                                                    float4* __restrict__ motion) {
    guide_pixel<false, true, true>(sc, cam, fa, samples, out, tri_prev, motion);
}

// the primitive-motion instances (TRI: a triangle snapshot is pending as well): plain, SDF, pixel filter
template <bool SDF, bool TRI>
__global__ __launch_bounds__(64) void guide_prim_motion_kernel(const DevScene sc, const DevCamera cam, const FrameArgs fa, unsigned samples,
                                                               float4* __restrict__ out, const TriGeom* __restrict__ tri_prev, const PrimPrev prims,
                                                               float4* __restrict__ motion) {
    guide_pixel<SDF, false, TRI, true>(sc, cam, fa, samples, out, tri_prev, motion, prims);
}
template <bool TRI>
__global__ __launch_bounds__(64) void filtered_guides_prim_motion_kernel(const DevScene sc, const DevCamera cam, const FrameArgs fa, unsigned samples,
                                                                         float4* __restrict__ out, const TriGeom* __restrict__ tri_prev,
                                                                         const PrimPrev prims, float4* __restrict__ motion) {
    guide_pixel<false, true, TRI, true>(sc, cam, fa, samples, out, tri_prev, motion, prims);
}

// one launcher for the plain and the motion instances (MOTION: tri_prev and motion are the two further kernel arguments)
template <bool SDF, bool FILTER, bool MOTION>
static void launch_guides_t(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                            float4* motion, hipStream_t stream) {
    const size_t lds = (size_t)sc.stack_levels * 64 * sizeof(unsigned);
    static size_t lds_attr = 0;
    const void* k;
    if constexpr (MOTION) k = FILTER ? reinterpret_cast<const void*>(&filtered_guides_motion_kernel) : reinterpret_cast<const void*>(&guide_motion_kernel<SDF>);
    else k = FILTER ? reinterpret_cast<const void*>(&filtered_guides_kernel) : reinterpret_cast<const void*>(&guide_kernel<SDF>);
    if (lds > 65536u && lds > lds_attr) {
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        lds_attr = lds;
    }
    const unsigned tiles = (unsigned)(((fa.width + 7) / 8) * ((fa.rows + 7) / 8));
    if constexpr (MOTION) {
        if constexpr (FILTER) hipLaunchKernelGGL(filtered_guides_motion_kernel, dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out, tri_prev, motion);
        else hipLaunchKernelGGL((guide_motion_kernel<SDF>), dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out, tri_prev, motion);
    } else {
        if constexpr (FILTER) hipLaunchKernelGGL(filtered_guides_kernel, dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out);
        else hipLaunchKernelGGL((guide_kernel<SDF>), dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out);
    }
}
template <bool MOTION>
static void launch_guides_m(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                            float4* motion, hipStream_t stream) {
    if (fa.filter_kind != PRT_FILTER_NONE) launch_guides_t<false, true, MOTION>(sc, cam, fa, samples, out, tri_prev, motion, stream);
    else if (sc.n_sdfs) launch_guides_t<true, false, MOTION>(sc, cam, fa, samples, out, tri_prev, motion, stream);
    else launch_guides_t<false, false, MOTION>(sc, cam, fa, samples, out, tri_prev, motion, stream);
}
void launch_guides(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, hipStream_t stream) {
    launch_guides_m<false>(sc, cam, fa, samples, out, nullptr, nullptr, stream);
}
void launch_guides_motion(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                          float4* motion, hipStream_t stream) {
    launch_guides_m<true>(sc, cam, fa, samples, out, tri_prev, motion, stream);
}

// the launcher of the primitive-motion instances
template <bool SDF, bool FILTER, bool TRI>
static void launch_guides_p(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                            const PrimPrev& prims, float4* motion, hipStream_t stream) {
    const size_t lds = (size_t)sc.stack_levels * 64 * sizeof(unsigned);
    static size_t lds_attr = 0;
    const void* k = FILTER ? reinterpret_cast<const void*>(&filtered_guides_prim_motion_kernel<TRI>) : reinterpret_cast<const void*>(&guide_prim_motion_kernel<SDF, TRI>);
    if (lds > 65536u && lds > lds_attr) {
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        lds_attr = lds;
    }
    const unsigned tiles = (unsigned)(((fa.width + 7) / 8) * ((fa.rows + 7) / 8));
    if constexpr (FILTER) hipLaunchKernelGGL((filtered_guides_prim_motion_kernel<TRI>), dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out, tri_prev, prims, motion);
    else hipLaunchKernelGGL((guide_prim_motion_kernel<SDF, TRI>), dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out, tri_prev, prims, motion);
}
template <bool TRI>
static void launch_guides_pt(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                             const PrimPrev& prims, float4* motion, hipStream_t stream) {
    if (fa.filter_kind != PRT_FILTER_NONE) launch_guides_p<false, true, TRI>(sc, cam, fa, samples, out, tri_prev, prims, motion, stream);
    else if (sc.n_sdfs) launch_guides_p<true, false, TRI>(sc, cam, fa, samples, out, tri_prev, prims, motion, stream);
    else launch_guides_p<false, false, TRI>(sc, cam, fa, samples, out, tri_prev, prims, motion, stream);
}
void launch_guides_prim_motion(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                               const PrimPrev& prims, float4* motion, hipStream_t stream) {
    if (tri_prev) launch_guides_pt<true>(sc, cam, fa, samples, out, tri_prev, prims, motion, stream);
    else launch_guides_pt<false>(sc, cam, fa, samples, out, nullptr, prims, motion, stream);
}

// ---- the filter ----------------------------------------------------------------------------------------------------------------------
PT_DEV float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
PT_DEV bool dn_finite3(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }
PT_DEV int dn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// var_source: 0 = stats plane {l, s2} with the path count of the state, 1 = 5x5 moments of the luminance (window clamped to the frame,
// non-finite colours left out)
__global__ __launch_bounds__(256) void dn_var_kernel(const float4* __restrict__ fb, const uint4* __restrict__ q4, const float2* __restrict__ adapt,
                                                     int spatial, int W, int H, float4* __restrict__ out) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    const float4 c = fb[id];
    float v = 0.0f;
    if (!spatial) {
        const unsigned n = q4[id].x;
        if (n >= 2u) {
            const float2 a = adapt[id];
            const float m = a.x / (float)n;
            v = fmaxf((a.y - a.x * m) / ((float)n * (float)(n - 1u)), 0.0f);
        }
    } else {
        float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
        for (int dy = -2; dy <= 2; ++dy)
            for (int dx = -2; dx <= 2; ++dx) {
                const float4 q = fb[(size_t)dn_clamp(y + dy, H - 1) * W + dn_clamp(x + dx, W - 1)];
                if (!dn_finite3(q)) continue;
                const float l = dn_lum(q.x, q.y, q.z);
                s1 += l; s2 += l * l; cnt += 1.0f;
            }
        if (cnt > 0.0f) { const float m = s1 / cnt; v = fmaxf(s2 / cnt - m * m, 0.0f); }
    }
    out[id] = make_float4(c.x, c.y, c.z, v);
}

__global__ __launch_bounds__(256) void dn_gauss_kernel(const float4* __restrict__ in, int W, int H, float* __restrict__ g) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    float s = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float w = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f) * 0.0625f;
            s += w * in[(size_t)dn_clamp(y + dy, H - 1) * W + dn_clamp(x + dx, W - 1)].w;
        }
    g[(size_t)y * W + x] = s;
}

struct DnParams { int step; float sigma_l, sigma_n, sigma_z, inv_sigma_a2; };

PT_DEV float dn_k(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

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

// alpha_src: null for every pass but the last, which writes {c', alpha of the framebuffer} instead of {c', v'}
__global__ __launch_bounds__(256) void dn_atrous_kernel(const float4* __restrict__ in, const float* __restrict__ g, const float4* __restrict__ gd,
                                                        int W, int H, const DnParams P, const float4* __restrict__ alpha_src,
                                                        float4* __restrict__ out) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    const float4 cp = in[id];
    float4 r = cp;
    if (dn_finite3(cp)) {
        const float4 ap = gd[2 * id], np = gd[2 * id + 1];
        const bool covp = ap.w > 0.0f;
        const float grad = covp ? fmaxf(dn_grad1(gd, x, y, 1, 0, W, H, np.w), dn_grad1(gd, x, y, 0, 1, W, H, np.w)) : 0.0f;
        const float lp = dn_lum(cp.x, cp.y, cp.z);
        const float l_den = P.sigma_l * sqrtf(g[id]) + 1e-6f;
        const float z_scale = P.sigma_z * grad * (float)P.step;
        float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * P.step;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * P.step;
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                const float4 cq = in[q];
                if (!dn_finite3(cq)) continue;
                const float4 aq = gd[2 * q], nq = gd[2 * q + 1];
                const bool covq = aq.w > 0.0f;
                float wn = 1.0f;
                if (covp && covq) wn = powf(fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z), P.sigma_n);
                else if (covp != covq) wn = 0.0f;
                const float wz = expf(-fabsf(np.w - nq.w) / (z_scale * sqrtf((float)(dx * dx + dy * dy)) + 1e-4f));
                const float da0 = ap.x - aq.x, da1 = ap.y - aq.y, da2 = ap.z - aq.z;
                const float wa = expf(-(da0 * da0 + da1 * da1 + da2 * da2) * P.inv_sigma_a2);
                const float wl = expf(-fabsf(lp - dn_lum(cq.x, cq.y, cq.z)) / l_den);
                const float w = (dx == 0 && dy == 0) ? 1.0f : wn * wz * wa * wl;
                if (!(w > 0.0f)) continue;                            // (a NaN weight -- guides without a normal -- drops the tap)
                const float hw = dn_k(dx) * dn_k(dy) * w;
                sw += hw;
                sr += hw * cq.x; sg += hw * cq.y; sb += hw * cq.z;
                sv += hw * hw * cq.w;
            }
        }
        const float inv = 1.0f / sw;
        r = make_float4(sr * inv, sg * inv, sb * inv, sv * (inv * inv));
    }
    if (alpha_src) r.w = alpha_src[id].w;
    out[id] = r;
}

// the filter's pieces for prt_denoise_temporal (pt_temporal.hip): {rgb, v} of the framebuffer into out, and a-trous pass i (its Gaussian
// into g first) from `in` to `out` -- alpha_src non-null for the last pass
void launch_denoise_var(const float4* fb, const uint4* q4, const float2* adapt, bool spatial, int W, int H, float4* out, hipStream_t stream) {
    const dim3 blk(16, 16), grd((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
    hipLaunchKernelGGL(dn_var_kernel, grd, blk, 0, stream, fb, q4, adapt, spatial ? 1 : 0, W, H, out);
}
void launch_denoise_pass(const float4* in, const float4* guides, int W, int H, const prt_denoise_params& p, unsigned i, float* g,
                         const float4* alpha_src, float4* out, hipStream_t stream) {
    const dim3 blk(16, 16), grd((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
    DnParams P;
    P.step = 1 << i; P.sigma_l = p.sigma_l; P.sigma_n = p.sigma_n; P.sigma_z = p.sigma_z; P.inv_sigma_a2 = 1.0f / (p.sigma_a * p.sigma_a);
    hipLaunchKernelGGL(dn_gauss_kernel, grd, blk, 0, stream, in, W, H, g);
    hipLaunchKernelGGL(dn_atrous_kernel, grd, blk, 0, stream, in, g, guides, W, H, P, alpha_src, out);
}

// passes of the filter: var -> (gauss, a-trous) x passes, ping-pong between buf0 and buf1, the last pass into `out` (rgba of the frame)
void launch_denoise(const float4* fb, const uint4* q4, const float2* adapt, bool spatial, const float4* guides, int W, int H,
                    const prt_denoise_params& p, float4* buf0, float4* buf1, float* g, float4* out, hipStream_t stream) {
    launch_denoise_var(fb, q4, adapt, spatial, W, H, buf0, stream);
    float4* cur = buf0;
    float4* nxt = buf1;
    for (unsigned i = 0; i < p.passes; ++i) {
        const bool last = i + 1 == p.passes;
        launch_denoise_pass(cur, guides, W, H, p, i, g, last ? fb : nullptr, last ? out : nxt, stream);
        float4* t = cur; cur = nxt; nxt = t;
    }
}

}  // namespace prt
