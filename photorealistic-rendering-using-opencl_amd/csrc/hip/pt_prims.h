// pt_prims.h -- the bodies of prt_update_primitives (pt_prims.hip; prt.h): prt_mesh records -> the DevSphere / DevSdf / DevQuad tables of
// pt_layout.h by pack_scene's own expressions, and where a hit point of a moved sphere, quad or SDF primitive was before the update(s)
// (prt.h prt_set_motion; the primitive-motion instances of the guide kernels in pt_denoise.hip).  Plain pointers and __host__ __device__
// inline functions only, as pt_refit.h / pt_motion.h, so that a host harness (tests/emu/prims_emu.cpp) runs the same code.  f32
// operations, no contraction (build.py: -ffp-contract=off); the divides and the square root are IEEE (correctly rounded).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>      // vector types of pt_layout.h

#include "pt_layout.h"
#include "pt_motion.h"

#if defined(__HIPCC__)
#define PT_PRIMS_HD __host__ __device__ inline
#else
#define PT_PRIMS_HD inline
#endif

namespace prt {

// a prt_mesh record (256 bytes, prt_types.h) as sixteen 16-byte accesses: pos is quad 4, joker quads 8 .. 11, t the low byte of quad 12
struct alignas(16) PrimQuad { float x, y, z, w; };
struct alignas(16) PrimWord { uint32_t x, y, z, w; };
constexpr uint32_t PT_MESH_QUADS = 16, PT_MESH_POS = 4, PT_MESH_JOKER = 8, PT_MESH_T = 12;

// |v| <= FLT_MAX is false for NaN and for the infinities
PT_PRIMS_HD bool prims_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e+38f; }

// record i of `meshes` (spheres first, then SDF primitives, then quads: pack_scene's order) into its table; types[i] is the uploaded
// record's t.  Returns true for a record that is refused: a different t, or a non-finite value in a field that is read (sphere: pos.xyz,
// joker[0]; SDF primitive: pos.xyz, joker[0..3]; quad: joker[0..12]).  A refused record may or may not have been written: the tables
// are staging tables
PT_PRIMS_HD bool prims_pack(const void* meshes, uint32_t i, uint32_t n_spheres, uint32_t n_sdfs, const uint8_t* types, DevSphere* spheres,
                            DevSdf* sdfs, DevQuad* quads) {
    const PrimQuad* q = reinterpret_cast<const PrimQuad*>(meshes) + (size_t)i * PT_MESH_QUADS;
    const PrimQuad pos = q[PT_MESH_POS];
    const PrimQuad j0 = q[PT_MESH_JOKER], j1 = q[PT_MESH_JOKER + 1], j2 = q[PT_MESH_JOKER + 2], j3 = q[PT_MESH_JOKER + 3];
    const uint32_t t = reinterpret_cast<const PrimWord*>(q)[PT_MESH_T].x & 0xFFu;
    bool bad = t != (uint32_t)types[i];
    if (i < n_spheres) {
        bad = bad || !(prims_finite(pos.x) && prims_finite(pos.y) && prims_finite(pos.z) && prims_finite(j0.x));
        *reinterpret_cast<PrimQuad*>(spheres + i) = PrimQuad{pos.x, pos.y, pos.z, j0.x};
    } else if (i < n_spheres + n_sdfs) {
        bad = bad || !(prims_finite(pos.x) && prims_finite(pos.y) && prims_finite(pos.z) && prims_finite(j0.x) && prims_finite(j0.y) &&
                       prims_finite(j0.z) && prims_finite(j0.w));
        DevSdf* d = sdfs + (i - n_spheres);
        reinterpret_cast<PrimWord*>(d)[0] = PrimWord{__builtin_bit_cast(uint32_t, pos.x), __builtin_bit_cast(uint32_t, pos.y),
                                                     __builtin_bit_cast(uint32_t, pos.z), t};
        reinterpret_cast<PrimQuad*>(d)[1] = j0;
    } else {
        const float j[13] = {j0.x, j0.y, j0.z, j0.w, j1.x, j1.y, j1.z, j1.w, j2.x, j2.y, j2.z, j2.w, j3.x};
        bool fin = true;
        for (int k = 0; k < 13; ++k) fin = fin && prims_finite(j[k]);
        bad = bad || !fin;
        DevQuad d;
        pack_quad(j, d);
        PrimQuad* o = reinterpret_cast<PrimQuad*>(quads + (i - n_spheres - n_sdfs));
        o[0] = PrimQuad{d.base[0], d.base[1], d.base[2], d.area};
        o[1] = PrimQuad{d.edge0[0], d.edge0[1], d.edge0[2], d.e0e0};
        o[2] = PrimQuad{d.edge1[0], d.edge1[1], d.edge1[2], d.e1e1};
        o[3] = PrimQuad{d.normal[0], d.normal[1], d.normal[2], d.u0};
        o[4] = PrimQuad{d.anchor[0], d.anchor[1], d.anchor[2], d.u1};
    }
    return bad;
}

// ---- where the hit point p of a primitive was before the update(s), minus where it is.  prev: the table as it was (the snapshot), cur: the
// table the ray was traced against.  Each is exactly +0 for an unchanged record

// sphere i: h = (p - c_cur) / |p - c_cur|; d = (c_prev - c_cur) + h * (r_prev - r_cur): translation and a change of radius
PT_PRIMS_HD MotionVec prims_sphere_displacement(const DevSphere* prev, const DevSphere* cur, uint32_t i, float px, float py, float pz) {
    const PrimQuad a = *reinterpret_cast<const PrimQuad*>(prev + i), c = *reinterpret_cast<const PrimQuad*>(cur + i);
    const float wx = px - c.x, wy = py - c.y, wz = pz - c.z;
    const float len = __builtin_sqrtf((wx * wx + wy * wy) + wz * wz);
    const float dr = a.w - c.w;
    MotionVec d;
    d.x = (a.x - c.x) + (wx / len) * dr;
    d.y = (a.y - c.y) + (wy / len) * dr;
    d.z = (a.z - c.z) + (wz / len) * dr;
    return d;
}

// quad j: w = p - anchor_cur (hit_quad measures from the anchor), a = dot(w, e0_cur) / e0e0_cur, b = dot(w, e1_cur) / e1e1_cur;
// q(rec) = (rec.anchor + rec.edge0 * a) + rec.edge1 * b; d = q(prev) - q(cur): translation, rotation and resizing of the card
PT_PRIMS_HD MotionVec prims_quad_point(const PrimQuad& e0, const PrimQuad& e1, const PrimQuad& an, float a, float b) {
    MotionVec q;
    q.x = (an.x + e0.x * a) + e1.x * b;
    q.y = (an.y + e0.y * a) + e1.y * b;
    q.z = (an.z + e0.z * a) + e1.z * b;
    return q;
}
PT_PRIMS_HD MotionVec prims_quad_displacement(const DevQuad* prev, const DevQuad* cur, uint32_t j, float px, float py, float pz) {
    const PrimQuad* cq = reinterpret_cast<const PrimQuad*>(cur + j);            // {base, area}, {edge0, e0e0}, {edge1, e1e1}, {normal, u0}, {anchor, u1}
    const PrimQuad* pq = reinterpret_cast<const PrimQuad*>(prev + j);
    const PrimQuad ce0 = cq[1], ce1 = cq[2], can = cq[4];
    const PrimQuad pe0 = pq[1], pe1 = pq[2], pan = pq[4];
    const float wx = px - can.x, wy = py - can.y, wz = pz - can.z;
    const float a = ((wx * ce0.x + wy * ce0.y) + wz * ce0.z) / ce0.w;
    const float b = ((wx * ce1.x + wy * ce1.y) + wz * ce1.z) / ce1.w;
    const MotionVec p = prims_quad_point(pe0, pe1, pan, a, b), q = prims_quad_point(ce0, ce1, can, a, b);
    MotionVec d;
    d.x = p.x - q.x; d.y = p.y - q.y; d.z = p.z - q.z;
    return d;
}

// SDF primitive k: d = pos_prev - pos_cur (translation only: a parameter change carries no motion)
PT_PRIMS_HD MotionVec prims_sdf_displacement(const DevSdf* prev, const DevSdf* cur, uint32_t k) {
    const PrimQuad a = *reinterpret_cast<const PrimQuad*>(prev + k), c = *reinterpret_cast<const PrimQuad*>(cur + k);
    MotionVec d;
    d.x = a.x - c.x; d.y = a.y - c.y; d.z = a.z - c.z;
    return d;
}

// the tables before the update(s), as the guide kernels' primitive-motion instances take them (a kernel argument of its own: DevScene is the
// render kernels' kernarg block)
struct PrimPrev { const DevSphere* spheres; const DevSdf* sdfs; const DevQuad* quads; };

// mesh index `mid` >= 0 of a scene with n_spheres spheres, then n_sdfs SDF primitives, then quads from quad_mesh_base on
PT_PRIMS_HD MotionVec prims_displacement(const PrimPrev& prev, const DevSphere* spheres, const DevSdf* sdfs, const DevQuad* quads, uint32_t n_spheres,
                                         uint32_t n_sdfs, uint32_t quad_mesh_base, uint32_t mid, float px, float py, float pz) {
    if (mid < n_spheres) return prims_sphere_displacement(prev.spheres, spheres, mid, px, py, pz);
    if (mid < n_spheres + n_sdfs) return prims_sdf_displacement(prev.sdfs, sdfs, mid - n_spheres);
    return prims_quad_displacement(prev.quads, quads, mid - quad_mesh_base, px, py, pz);
}

}  // namespace prt
