// pt_guides.h -- feature buffers ("guides") of prt_render_guides (include/prt.h): first non-delta hit albedo, coverage, normal, depth.
// No counterpart in the reference (its VIEW_ALBEDO is a name without a branch, kernels/main.cl:6-15).  Device functions only; the
// kernel is guide_kernel in pt_denoise.hip.
//
// One lane per pixel, 8x8 tiles per 64-lane wave as in render_kernel, global pixel coordinates.  A lane walks each of its rays to the end
// with the render kernel's walk steps (walk_begin / walk_box / walk_tri, pt_device.h) and finish_closest; primary rays and their few delta
// bounces are coherent, so there is no phase scheduling.  The arithmetic is ordinary f32: the guides are compared with a float64 caster,
// not with a bit-exact oracle.
#pragma once
#include "pt_device.h"

namespace prt {
namespace dev {

#define PT_GUIDE_MAX_DELTA 4        // delta events (smooth conductor reflections, smooth dielectric refractions) a guide ray follows

// prt.h prt_render_guides: sample s of a pixel sits at the fractional offset (0.5, 0.5) for s = 0, else at the R2 point
// ((0.5 + s a1) mod 1, (0.5 + s a2) mod 1); the lens sample is the same pair shifted by (0.25, 0.75) mod 1
PT_DEV float guide_frac(float x) { return x - prt_floor(x); }
PT_DEV void guide_offsets(unsigned s, float& fx, float& fy) {
    fx = s ? guide_frac(0.5f + (float)s * 0.7548776662f) : 0.5f;
    fy = s ? guide_frac(0.5f + (float)s * 0.5698402910f) : 0.5f;
}

// create_cam_ray (pt_device.h) with explicit sample values instead of RNG draws: the image-plane point of (cx + ox, cy + oy) and, with
// an aperture, the lens point of (lx, ly) in [0, 1)^2
PT_DEV Ray guide_cam_ray_at(int cx, int cy, int width, int height, const DevCamera& cam, float ox, float oy, float lx, float ly) {
    const f3 hAxis = ld3(cam.hAxis), vAxis = ld3(cam.vAxis), position = ld3(cam.position);
    const f3 middle = ld3(cam.middle), horizontal = ld3(cam.horizontal), vertical = ld3(cam.vertical);
    const float px = (float)cx + ox;
    const float py = (float)(height - cy - 1) - oy;
    const float sx = px / (width - 1.0f);
    const float sy = py / (height - 1.0f);
    const f3 onPlane = middle + (horizontal * ((2 * sx) - 1)) + (vertical * ((2 * sy) - 1));
    const f3 onImagePlane = position + ((onPlane - position) * cam.focalDistance);
    f3 aperturePoint = position;
    if (cam.apertureRadius > 0.00001f) {
        const float angle = 2 * PT_PI * lx;
        const float distance = cam.apertureRadius * hw_sqrt(ly);
        float sn, cs;
        sincos_pair(angle, sn, cs);
        aperturePoint = position + (hAxis * (cs * distance)) + (vAxis * (sn * distance));
    }
    Ray ray;
    ray.backside = false;
    ray.origin = aperturePoint;
    ray.dir = normalize(onImagePlane - aperturePoint);
    ray.time = 0.0f;
    ray.normal = splat(0.0f);
    ray.pos = splat(0.0f);
    ray.t = 0.0f;
    return ray;
}
// ... at the sample's fractional position (fx, fy): the offset (fx - 0.5, fy - 0.5)
PT_DEV Ray guide_cam_ray(int cx, int cy, int width, int height, const DevCamera& cam, float fx, float fy, float lx, float ly) {
    return guide_cam_ray_at(cx, cy, width, height, cam, fx - 0.5f, fy - 0.5f, lx, ly);
}

// closest hit of `ray` against the whole scene: the tree walked to its end, then finish_closest.  Out: ray.t / pos / normal / backside,
// and th: the tree's closest triangle (the hit itself when mesh_id comes out -1 and the ray hit)
template <bool SDF>
PT_DEV bool guide_trace(const DevScene& sc, Ray& ray, const TravStack& stk, int& mesh_id, TriHit& th) {
    const RayPre p = ray_pre(ray);
    WalkState w;
    walk_begin(sc, false, ray, PT_INF, p, w, stk);
    while (!w.done) {
        if (w.pend_count) walk_tri(sc, false, ray, w);
        else walk_box(sc, false, ray, p, w, stk);
    }
    TravRes r;
    r.found = w.found; r.t = w.t; r.th.u = w.u; r.th.v = w.v; r.th.slot = w.slot;
    th = r.th;
    return finish_closest<SDF>(sc, ray, r, mesh_id);
}

PT_DEV f3 clamp01(f3 c) {
    return F3(prt_fmin(prt_fmax(c.x, 0.0f), 1.0f), prt_fmin(prt_fmax(c.y, 0.0f), 1.0f), prt_fmin(prt_fmax(c.z, 0.0f), 1.0f));
}

// direct_triangle: the hit that gives the values is the ray's FIRST (no delta event before it) and a mesh triangle (the one that wins
// finish_closest: mesh_id == -1); then {slot, u, v} name it (prt.h prt_set_motion: the samples that carry motion)
// direct_prim: the FIRST hit is a sphere, an SDF primitive or a quad (mesh_id >= 0); then {mid, pos} name it (prt.h prt_update_primitives)
struct GuideSample { f3 albedo, normal; float depth; bool hit; unsigned slot; float u, v; bool direct_triangle; bool direct_prim; int mid; f3 pos; };

// one guide sample along `ray` (prt.h: the delta chain, the per-hit values, the miss)
template <bool SDF>
PT_DEV GuideSample guide_sample(const DevScene& sc, Ray ray, const TravStack& stk) {
    GuideSample g;
    g.normal = splat(0.0f); g.depth = 0.0f; g.hit = false;
    g.slot = 0u; g.u = 0.0f; g.v = 0.0f; g.direct_triangle = false;
    g.direct_prim = false; g.mid = -1; g.pos = splat(0.0f);
    f3 tint = splat(1.0f);
    float dist = 0.0f;
    for (int events = 0;; ++events) {
        ray.normal = splat(0.0f);
        int mid;
        TriHit th;
        if (!guide_trace<SDF>(sc, ray, stk, mid, th)) {
            g.albedo = tint * clamp01(env_lookup(sc, ray.dir));
            return g;
        }
        dist = dist + ray.t;
        const Mat mat = load_mat(sc.mats, (mid + 1) ? (unsigned)(mid + 1) : sc.n_meshes + 1u);
        const bool cond = (mat.t & PRT_MAT_COND) && !(mat.t & PRT_MAT_ROUGH_COND);
        const bool diel = (mat.t & PRT_MAT_DIEL) && !(mat.t & PRT_MAT_ROUGH_DIEL);
        if (!(cond || diel) || events == PT_GUIDE_MAX_DELTA) {
            g.albedo = tint * clamp01(mat.color);
            g.normal = dot(ray.normal, ray.dir) > 0.0f ? -ray.normal : ray.normal;
            g.depth = dist;
            g.hit = true;
            g.direct_triangle = events == 0 && mid == -1;
            g.slot = th.slot; g.u = th.u; g.v = th.v;
            g.direct_prim = events == 0 && mid >= 0;
            g.mid = mid; g.pos = ray.pos;
            return g;
        }
        const f3 n = ray.normal;                                  // the shading normal as finish_closest leaves it (what bsdf sampling frames)
        const float c = -dot(n, ray.dir);                         // wi.z of the scatter event
        f3 d = ray.dir - n * (2.0f * dot(ray.dir, n));            // mirror reflection
        if (cond) {
            tint = tint * clamp01(mat.color);
        } else {
            const float eta = c < 0.0f ? mat.eta.x : hw_recip(mat.eta.x);   // dielectric_sample's index
            float cosT = 0.0f;
            const float F = dielectric_reflectance(eta, prt_fabs(c), cosT);
            if (F != 1.0f) d = (ray.dir + n * c) * eta - n * prt_copysign(cosT, c);   // refraction (reflection on total internal reflection)
        }
        ray.origin = ray.pos;
        ray.dir = normalize(d);
    }
}

}  // namespace dev
}  // namespace prt
