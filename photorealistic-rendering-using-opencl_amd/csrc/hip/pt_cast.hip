// pt_cast.hip -- ray queries (prt_cast_rays, prt_occluded, prt_cast_pixels; include/prt.h has the contract; the per-ray bodies are
// pt_cast.h).  A translation unit of its own: no code object of the render kernels changes with it.
//
//   cast_kernel<SDF, ANY>    one lane per ray, 64-lane workgroups: ray i is lane i % 64 of workgroup i / 64.  ANY: the occlusion test
//   cast_pixel_rays_kernel   the rays of prt_cast_pixels into the staging buffer
//
// The walk stack is in dynamic LDS as in guide_kernel: sc.stack_levels x 64 words, [level][lane].
//
// The callers' rays are not coherent the way primary rays are, so the walk loop is render_kernel's walk phase (pt_render_body.h) without its
// cut: a lane without a pending triangle takes a box step; the triangle unit runs once PT_CAST_TRI_SIXTEENTHS sixteenths of the lanes
// still walking have a triangle pending -- which includes the case that no lane can take a box step.  Each lane's sequence of steps is
// its own whatever the wave does: no bit of a result depends on the schedule (tests/test_cast_rays.py shuffles the rays).
// -DPT_CAST_PLAIN_LOOP builds the per-lane loop of guide_trace instead, for the measurement of tools/cast_rate.py (DESIGN.md s4 "Ray queries").
#include "pt_cast.h"
#include "pt_launch.h"

namespace prt {
using namespace dev;

#define PT_CAST_TRI_SIXTEENTHS 4u

template <bool SDF, bool ANY>
__global__ __launch_bounds__(64) void cast_kernel(const DevScene sc, const float4* __restrict__ rays, unsigned n,
                                                  const uint32_t* __restrict__ slot_vtx, void* __restrict__ out) {
    extern __shared__ unsigned lds_stack[];                     // sc.stack_levels x 64, sized by the launch
    TravStack stk;
    stk.lds = lds_stack + threadIdx.x; stk.stride = 64;
    const unsigned i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
#ifdef PT_CAST_PLAIN_LOOP
    cast_one<SDF, ANY>(sc, rays, i, slot_vtx, out, stk);
#else
    CastLane L;
    const bool valid = cast_begin(sc, ANY, rays, i, L, stk);
    if (!L.w.done) {
        for (;;) {
            if (!L.w.pend_count) walk_box(sc, ANY, L.ray, L.p, L.w, stk);
            const bool pending = L.w.pend_count != 0u;
            const unsigned n_in = (unsigned)__popcll(__ballot(1)), n_pend = (unsigned)__popcll(__ballot(pending));
            if (pending && n_pend * 16u >= n_in * PT_CAST_TRI_SIXTEENTHS) walk_tri(sc, ANY, L.ray, L.w);
            if (L.w.done) break;
        }
    }
    if constexpr (ANY) {
        if (valid) cast_store_occluded<SDF>(sc, L, static_cast<uint32_t*>(out), i);
        else static_cast<uint32_t*>(out)[i] = 0u;
    } else {
        if (valid) cast_store_hit<SDF>(sc, L, slot_vtx, static_cast<float4*>(out), i);
        else cast_store_miss(static_cast<float4*>(out), i);
    }
#endif
}

__global__ __launch_bounds__(64) void cast_pixel_rays_kernel(const DevCamera cam, int width, int full_height, const int32_t* __restrict__ xy,
                                                             unsigned n, float4* __restrict__ rays) {
    const unsigned i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) cast_pixel_ray(cam, width, full_height, xy, i, rays);
}

template <bool SDF, bool ANY>
static void launch_cast_t(const DevScene& sc, const float4* rays, uint32_t n, const uint32_t* slot_vtx, void* out, hipStream_t stream) {
    const size_t lds = (size_t)sc.stack_levels * 64 * sizeof(unsigned);
    static size_t lds_attr = 0;
    if (lds > 65536u && lds > lds_attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cast_kernel<SDF, ANY>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        lds_attr = lds;
    }
    hipLaunchKernelGGL((cast_kernel<SDF, ANY>), dim3((n + 63u) / 64u), dim3(64), lds, stream, sc, rays, n, slot_vtx, out);
}

void launch_cast(const DevScene& sc, bool any_hit, const void* rays, uint32_t n, const uint32_t* slot_vtx, void* out, hipStream_t stream) {
    const float4* r = static_cast<const float4*>(rays);
    if (n == 0) return;
    if (sc.n_sdfs) {
        if (any_hit) launch_cast_t<true, true>(sc, r, n, slot_vtx, out, stream);
        else launch_cast_t<true, false>(sc, r, n, slot_vtx, out, stream);
    } else {
        if (any_hit) launch_cast_t<false, true>(sc, r, n, slot_vtx, out, stream);
        else launch_cast_t<false, false>(sc, r, n, slot_vtx, out, stream);
    }
}

void launch_cast_pixel_rays(const DevCamera& cam, int width, int full_height, const int32_t* xy, uint32_t n, void* rays, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(cast_pixel_rays_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, cam, width, full_height, xy, n, static_cast<float4*>(rays));
}

}  // namespace prt
