// pt_motion.h -- the bodies of the motion plane (prt.h prt_set_motion; the motion instances of the guide kernels in pt_denoise.hip): where a
// hit point of the deforming mesh was before the last update(s), from the triangle records of the previous geometry (the snapshot
// prt_update_vertices keeps) and the current ones.  A refit keeps the topology: slot s, barycentrics (u, v) name the same material point in
// both.  Plain pointers and __host__ __device__ inline functions only, as pt_refit.h, so that a host harness (tests/emu/motion_emu.cpp) runs
// the same code.  f32 operations, no contraction (build.py: -ffp-contract=off).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>      // vector types of pt_layout.h

#include "pt_layout.h"

#if defined(__HIPCC__)
#define PT_MOTION_HD __host__ __device__ inline
#else
#define PT_MOTION_HD inline
#endif

namespace prt {

struct alignas(16) MotionQuad { float x, y, z, w; };      // one 16-byte access: a third of a TriGeom, a pixel of the motion plane
struct MotionVec { float x, y, z; };

// q(rec) = (p0 - e1 u) + e2 v per component: p1 = p0 - e1, p2 = p0 + e2; u weighs vertex 1, v vertex 2 (as finish_closest's normal)
PT_MOTION_HD MotionVec motion_point(const TriGeom* rec, float u, float v) {
    const MotionQuad* g = reinterpret_cast<const MotionQuad*>(rec);                     // {p0, e1.x}, {e1.yz, e2.xy}, {e2.z, n}
    const MotionQuad a = g[0], b = g[1], c = g[2];
    MotionVec q;
    q.x = (a.x - a.w * u) + b.z * v;
    q.y = (a.y - b.x * u) + b.w * v;
    q.z = (a.z - b.y * u) + c.x * v;
    return q;
}

// d_s = q(tri_prev[slot]) - q(tri_geom[slot]): where the point was, minus where it is.  Exactly +0 for an unchanged record
PT_MOTION_HD MotionVec motion_displacement(const TriGeom* tri_prev, const TriGeom* tri_geom, uint32_t slot, float u, float v) {
    const MotionVec p = motion_point(tri_prev + slot, u, v), q = motion_point(tri_geom + slot, u, v);
    MotionVec d;
    d.x = p.x - q.x; d.y = p.y - q.y; d.z = p.z - q.z;
    return d;
}

// the per-pixel reduction: the contributing samples' displacements summed in sample order, their number counted
struct MotionSum { float x, y, z; uint32_t n; };
PT_MOTION_HD MotionSum motion_sum_begin() { return MotionSum{0.0f, 0.0f, 0.0f, 0u}; }
PT_MOTION_HD void motion_sum_add(MotionSum& s, const MotionVec& d) {
    s.x = s.x + d.x; s.y = s.y + d.y; s.z = s.z + d.z;
    ++s.n;
}
// {D, m}: D = sum / (float)hits (the guides' own hit count: the mean over the hits, as the guides' depth), m = contributing / samples
// with the guides' 1 / samples; hits == 0: zeros
PT_MOTION_HD MotionQuad motion_pixel(const MotionSum& s, uint32_t hits, uint32_t samples) {
    if (hits == 0u) return MotionQuad{0.0f, 0.0f, 0.0f, 0.0f};
    const float h = (float)hits;
    const float inv_k = 1.0f / (float)samples;
    return MotionQuad{s.x / h, s.y / h, s.z / h, (float)s.n * inv_k};
}

}  // namespace prt
