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
#include "pt_denoise_dev.h"
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

// the launch of any instance: one wave per 8x8 tile, the walk stack in LDS -- beyond 64 KiB of it (more than 256 stack levels) the kernel is
// told first.  tail: the kernel's arguments behind `out`
template <typename Kernel, typename... Tail>
static void launch_guide_kernel(Kernel kernel, const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out,
                                hipStream_t stream, Tail... tail) {
    const size_t lds = (size_t)sc.stack_levels * 64 * sizeof(unsigned);
    if (lds > 65536u) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const unsigned tiles = (unsigned)(((fa.width + 7) / 8) * ((fa.rows + 7) / 8));
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(64), lds, stream, sc, cam, fa, samples, out, tail...);
}
// the instance by pixel filter (which excludes SDF scenes), SDF primitives, and the pending snapshots of triangles and of primitives.  (The
// template instances stand in the code object in the order they are named here)
void launch_guides(const DevScene& sc, const DevCamera& cam, const FrameArgs& fa, unsigned samples, float4* out, const TriGeom* tri_prev,
                   const PrimPrev* prims, float4* motion, hipStream_t stream) {
    const bool filter = fa.filter_kind != PRT_FILTER_NONE, sdf = !filter && sc.n_sdfs;
    const auto go = [&](auto kernel, auto... tail) { launch_guide_kernel(kernel, sc, cam, fa, samples, out, stream, tail...); };
    if (!prims && !tri_prev) {
        if (filter) go(&filtered_guides_kernel);
        else if (!sdf) go(&guide_kernel<false>);
        else go(&guide_kernel<true>);
    } else if (!prims) {
        if (filter) go(&filtered_guides_motion_kernel, tri_prev, motion);
        else if (!sdf) go(&guide_motion_kernel<false>, tri_prev, motion);
        else go(&guide_motion_kernel<true>, tri_prev, motion);
    } else if (tri_prev) {
        if (filter) go(&filtered_guides_prim_motion_kernel<true>, tri_prev, *prims, motion);
        else if (!sdf) go(&guide_prim_motion_kernel<false, true>, tri_prev, *prims, motion);
        else go(&guide_prim_motion_kernel<true, true>, tri_prev, *prims, motion);
    } else {
        if (filter) go(&filtered_guides_prim_motion_kernel<false>, tri_prev, *prims, motion);
        else if (!sdf) go(&guide_prim_motion_kernel<false, false>, tri_prev, *prims, motion);
        else go(&guide_prim_motion_kernel<true, false>, tri_prev, *prims, motion);
    }
}

// ---- the filter ----------------------------------------------------------------------------------------------------------------------
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
        v = dn_stats_var(q4, adapt, id);
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

// ---- the chain: variance -> [reprojection, clamp] -> (gauss, a-trous) x passes ------------------------------------------------------------
// The passes ping-pong from buf0 to buf1 and back.  So the frame's {rgb, v} goes into buf0 where the passes read it first, and into buf1 where
// the reprojection stands in between: it reads {rgb, v} there and writes the passes' input into buf0.  Nobody else knows which
static float4* var_plane(const FilterPlanes& pl, bool temporal) { return temporal ? pl.buf1 : pl.buf0; }

void launch_filter_variance(const FilterPlanes& pl, bool temporal, const VarianceSource& src, hipStream_t stream) {
    float4* var = var_plane(pl, temporal);
    if (src.records) launch_records_import(src.records, pl.W, pl.H, pl.fb, pl.guides, var, src.no_stats, stream);
    else hipLaunchKernelGGL(dn_var_kernel, dn_grid(pl.W, pl.H), dn_block(), 0, stream, pl.fb, src.q4, src.adapt, src.spatial ? 1 : 0, pl.W, pl.H, var);
}

void launch_filter_chain(const FilterPlanes& pl, const prt_denoise_params& p, const prt_temporal_params* t, const DevCamera* cam,
                         const TemporalHistory* h, const float4* motion, hipStream_t stream) {
    const dim3 blk = dn_block(), grd = dn_grid(pl.W, pl.H);
    if (t) launch_temporal_front(pl, var_plane(pl, true), pl.buf0, *t, *cam, *h, motion, stream);
    DnParams P;
    P.sigma_l = p.sigma_l; P.sigma_n = p.sigma_n; P.sigma_z = p.sigma_z; P.inv_sigma_a2 = 1.0f / (p.sigma_a * p.sigma_a);
    float4* cur = pl.buf0;
    float4* nxt = pl.buf1;
    for (unsigned i = 0; i < p.passes; ++i) {
        // pass i: step 2^i, the Gaussian of v first; the last one writes the frame's rgba -- its colour with the framebuffer's alpha
        const bool last = i + 1 == p.passes;
        float4* dst = last ? pl.out : nxt;
        P.step = 1 << i;
        hipLaunchKernelGGL(dn_gauss_kernel, grd, blk, 0, stream, cur, pl.W, pl.H, pl.g);
        hipLaunchKernelGGL(dn_atrous_kernel, grd, blk, 0, stream, cur, pl.g, pl.guides, pl.W, pl.H, P, last ? pl.fb : nullptr, dst);
        if (i == 0 && t && t->feedback == PRT_TEMPORAL_FEEDBACK_ATROUS) launch_temporal_feedback(dst, pl.W, pl.H, h->cn, stream);
        float4* tmp = cur; cur = nxt; nxt = tmp;
    }
}

}  // namespace prt
