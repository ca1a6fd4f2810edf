// pt_cast.h -- ray queries (prt_cast_rays, prt_occluded, prt_cast_pixels; include/prt.h has the contract): the per-ray bodies.  No
// counterpart in the reference.  Device functions on plain pointers; the kernels are in pt_cast.hip, and tests/emu/cast_emu.cpp compiles
// the same text for the host (-DPT_EMU).
//
// A query sees what a path segment of the render sees: the closest hit is ray_pre, walk_begin, the walk to its end and finish_closest --
// guide_trace of pt_guides.h with the caller's limit --, the occlusion test the render's shadow(): the any-hit walk, then finish_shadow.
// The bodies come in three pieces so that a wave can schedule the walk steps of its lanes (pt_cast.hip): cast_begin reads and validates
// one ray and takes the step at the root, the caller runs walk_box / walk_tri until w.done, cast_store_hit / cast_store_occluded finish
// the ray and write its record.  cast_walk is the plain per-lane loop between the two.
#pragma once
#include "pt_guides.h"

namespace prt {
namespace dev {

#define PT_HIT_MISS (-2)                // prt.h PRT_HIT_MISS / PRT_HIT_TRIANGLE
#define PT_HIT_TRIANGLE (-1)

struct CastLane {
    Ray ray;
    RayPre p;
    float limit;
    WalkState w;
};

PT_DEV bool cast_finite(float x) { return (prt_f2u(x) & 0x7f800000u) != 0x7f800000u; }

// prt.h "Invalid rays": a non-finite origin or direction, an all-zero direction, tmax NaN or <= 0
PT_DEV bool cast_ray_valid(const float4 o, const float4 d) {
    const bool fin = cast_finite(o.x) && cast_finite(o.y) && cast_finite(o.z) && cast_finite(d.x) && cast_finite(d.y) && cast_finite(d.z);
    const bool nonzero = d.x != 0.0f || d.y != 0.0f || d.z != 0.0f;
    return fin && nonzero && o.w > 0.0f;
}

// ray i of `rays` (prt_ray: {origin, tmax}, {dir, pad}) into L, and the step at the root.  false: an invalid ray, nothing was walked
// (L.w.done is set: the lane takes no step)
PT_DEV bool cast_begin(const DevScene& sc, const bool ANY_HIT, const float4* __restrict__ rays, size_t i, CastLane& L, const TravStack& stk) {
    const float4 o = rays[2 * i], d = rays[2 * i + 1];
    L.w.done = true; L.w.pend_count = 0;
    if (!cast_ray_valid(o, d)) return false;
    L.limit = o.w < PT_INF ? o.w : PT_INF;
    L.ray.backside = false;
    L.ray.origin = F3(o.x, o.y, o.z);
    L.ray.dir = F3(d.x, d.y, d.z);
    L.ray.time = 0.0f;
    L.ray.normal = splat(0.0f);
    L.ray.pos = splat(0.0f);
    L.ray.t = ANY_HIT ? L.limit : 0.0f;             // (the any-hit steps read their limit from ray.t)
    L.p = ray_pre(L.ray);
    walk_begin(sc, ANY_HIT, L.ray, L.limit, L.p, L.w, stk);
    return true;
}

// the plain per-lane loop (guide_trace's)
PT_DEV void cast_walk(const DevScene& sc, const bool ANY_HIT, CastLane& L, const TravStack& stk) {
    while (!L.w.done) {
        if (L.w.pend_count) walk_tri(sc, ANY_HIT, L.ray, L.w);
        else walk_box(sc, ANY_HIT, L.ray, L.p, L.w, stk);
    }
}

// record i of `hits` (prt_hit, 48 bytes) as three 16-byte stores
PT_DEV void cast_store_record(float4* __restrict__ hits, size_t i, float t, float u, float v, unsigned tri, f3 n, int id, f3 pos, unsigned flags) {
    hits[3 * i] = make_float4(t, u, v, prt_u2f(tri));
    hits[3 * i + 1] = make_float4(n.x, n.y, n.z, prt_u2f((unsigned)id));
    hits[3 * i + 2] = make_float4(pos.x, pos.y, pos.z, prt_u2f(flags));
}
PT_DEV void cast_store_miss(float4* __restrict__ hits, size_t i) {
    cast_store_record(hits, i, 0.0f, 0.0f, 0.0f, 0u, splat(0.0f), PT_HIT_MISS, splat(0.0f), 0u);
}

// the walk of a valid ray is over: finish_closest and the record.  slot_vtx: first vertex of every slot's triangle in the caller's arrays
// (read for a triangle hit only: a scene without triangles has none)
template <bool SDF>
PT_DEV void cast_store_hit(const DevScene& sc, CastLane& L, const uint32_t* __restrict__ slot_vtx, float4* __restrict__ hits, size_t i) {
    TravRes r;
    r.found = L.w.found; r.t = L.w.t; r.th.u = L.w.u; r.th.v = L.w.v; r.th.slot = L.w.slot;
    int mesh_id;
    finish_closest<SDF>(sc, L.ray, r, mesh_id);
    if (!(L.ray.t < L.limit)) { cast_store_miss(hits, i); return; }
    const bool tri = mesh_id == -1;
    cast_store_record(hits, i, L.ray.t, tri ? r.th.u : 0.0f, tri ? r.th.v : 0.0f, tri ? slot_vtx[r.th.slot] / 3u : 0u, L.ray.normal,
                      tri ? PT_HIT_TRIANGLE : mesh_id, L.ray.pos, L.ray.backside ? 1u : 0u);
}

// ... of the any-hit walk: the rest of shadow() when the tree did not occlude, and the flag
template <bool SDF>
PT_DEV void cast_store_occluded(const DevScene& sc, const CastLane& L, uint32_t* __restrict__ out, size_t i) {
    bool occluded = L.w.found;
    if (!occluded) occluded = !finish_shadow<SDF>(sc, L.ray.origin, L.ray.dir, L.limit);
    out[i] = occluded ? 1u : 0u;
}

// one ray from its record to its result, the plain loop in between: what a lane does when nothing schedules the wave
template <bool SDF, bool ANY_HIT>
PT_DEV void cast_one(const DevScene& sc, const float4* __restrict__ rays, size_t i, const uint32_t* __restrict__ slot_vtx, void* __restrict__ out,
                     const TravStack& stk) {
    CastLane L;
    const bool valid = cast_begin(sc, ANY_HIT, rays, i, L, stk);
    if (valid) cast_walk(sc, ANY_HIT, L, stk);
    if (ANY_HIT) {
        if (valid) cast_store_occluded<SDF>(sc, L, static_cast<uint32_t*>(out), i);
        else static_cast<uint32_t*>(out)[i] = 0u;
    } else {
        if (valid) cast_store_hit<SDF>(sc, L, slot_vtx, static_cast<float4*>(out), i);
        else cast_store_miss(static_cast<float4*>(out), i);
    }
}

// prt_cast_pixels: the ray of pixel xy[2 i], xy[2 i + 1] (full-frame coordinates) into rays[i] -- the centre ray of the pixel through the
// middle of the lens (guide_cam_ray_at at offset 0 with the aperture point at the camera's position; for a pinhole camera guide sample 0),
// tmax = PT_INF.  A pixel outside the frame gets a ray with tmax = 0, which the cast reports as a miss
PT_DEV void cast_pixel_ray(DevCamera cam, int width, int full_height, const int32_t* __restrict__ xy, size_t i, float4* __restrict__ rays) {
    const int x = xy[2 * i], y = xy[2 * i + 1];
    if (x < 0 || y < 0 || x >= width || y >= full_height) {
        rays[2 * i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rays[2 * i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    cam.apertureRadius = 0.0f;
    const Ray r = guide_cam_ray_at(x, y, width, full_height, cam, 0.0f, 0.0f, 0.0f, 0.0f);
    rays[2 * i] = make_float4(r.origin.x, r.origin.y, r.origin.z, PT_INF);
    rays[2 * i + 1] = make_float4(r.dir.x, r.dir.y, r.dir.z, 0.0f);
}

}  // namespace dev
}  // namespace prt
