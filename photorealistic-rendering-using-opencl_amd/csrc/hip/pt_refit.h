// pt_refit.h -- the bodies of the refit kernels (pt_refit.hip; prt.h prt_update_vertices): new vertices -> the triangle records of every slot
// and the boxes of every NodePair, the tree's topology kept.  Plain pointers and __host__ __device__ inline functions only, so that a host
// harness (tests/emu/refit_emu.cpp) runs the same code serially.  f32 operations, no contraction (build.py: -ffp-contract=off); boxes are
// comparisons only, hence exact.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>      // vector types of pt_layout.h

#include "pt_layout.h"

#if defined(__HIPCC__)
#define PT_REFIT_HD __host__ __device__ inline
#else
#define PT_REFIT_HD inline
#endif

namespace prt {

// one 16-byte access (a dwordx4 load or store on the device): vertices, normals, TriGeom / TriNrm thirds, NodePair quarters
struct alignas(16) RefitQuad { float x, y, z, w; };
struct alignas(16) RefitMeta { uint32_t m[4]; };

// x, y and z of vertex i are finite (lane 3 is not looked at: the reference never reads it)
PT_REFIT_HD bool refit_vertex_finite(const float* vertices, size_t i) {
    const RefitQuad v = reinterpret_cast<const RefitQuad*>(vertices)[i];
    // |x| <= FLT_MAX is false for NaN and for the infinities
    return __builtin_fabsf(v.x) <= 3.4028234663852886e+38f && __builtin_fabsf(v.y) <= 3.4028234663852886e+38f && __builtin_fabsf(v.z) <= 3.4028234663852886e+38f;
}

// the records of slot s (pt_pack.cpp pack_scene, "triangles in slot order": the same expressions).  normals null: TriNrm is not touched
PT_REFIT_HD void refit_tri(const float* vertices, const float* normals, const uint32_t* slot_vtx, size_t s, TriGeom* tri_geom, TriNrm* tri_nrm) {
    const uint32_t fv = slot_vtx[s];
    const RefitQuad* v = reinterpret_cast<const RefitQuad*>(vertices) + fv;
    const RefitQuad p0 = v[0], p1 = v[1], p2 = v[2];
    const float e1x = p0.x - p1.x, e1y = p0.y - p1.y, e1z = p0.z - p1.z;                // triangle.cl:12-13
    const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
    const float nx = e1y * e2z - e1z * e2y;                                             // triangle.cl:15
    const float ny = e1z * e2x - e1x * e2z;
    const float nz = e1x * e2y - e1y * e2x;
    RefitQuad* g = reinterpret_cast<RefitQuad*>(tri_geom + s);                          // {p0, e1.x}, {e1.yz, e2.xy}, {e2.z, n}
    g[0] = RefitQuad{p0.x, p0.y, p0.z, e1x};
    g[1] = RefitQuad{e1y, e1z, e2x, e2y};
    g[2] = RefitQuad{e2z, nx, ny, nz};
    if (normals) {
        const RefitQuad* n = reinterpret_cast<const RefitQuad*>(normals) + fv;
        const RefitQuad n0 = n[0], n1 = n[1], n2 = n[2];
        RefitQuad* t = reinterpret_cast<RefitQuad*>(tri_nrm + s);
        t[0] = RefitQuad{n0.x, n0.y, n0.z, 0.0f};
        t[1] = RefitQuad{n1.x, n1.y, n1.z, 0.0f};
        t[2] = RefitQuad{n2.x, n2.y, n2.z, 0.0f};
    }
}

// a box as the six floats of prt_bvh_node::bounds and of a NodePair child: min_x max_x min_y max_y min_z max_z
struct RefitBox { float b[6]; };

// merges the point or the box {lo, hi} per axis into `a` -- std::min / std::max as csrc/host/bvh.cpp uses them: the comparison form fixes
// which zero a bound of +0.0 and -0.0 keeps (the one that came first)
PT_REFIT_HD void refit_merge(RefitBox& a, float lox, float hix, float loy, float hiy, float loz, float hiz) {
    a.b[0] = lox < a.b[0] ? lox : a.b[0]; a.b[1] = hix > a.b[1] ? hix : a.b[1];
    a.b[2] = loy < a.b[2] ? loy : a.b[2]; a.b[3] = hiy > a.b[3] ? hiy : a.b[3];
    a.b[4] = loz < a.b[4] ? loz : a.b[4]; a.b[5] = hiz > a.b[5] ? hiz : a.b[5];
}

// the leaf rule: the box of the slots first .. first + count - 1, vertices 0, 1, 2 of each in slot order.  count == 0: `keep`
PT_REFIT_HD RefitBox refit_leaf_box(const float* vertices, const uint32_t* slot_vtx, uint32_t first, uint32_t count, const RefitBox& keep) {
    if (count == 0) return keep;
    RefitBox a;
    for (uint32_t j = 0; j < count; ++j) {
        const RefitQuad* v = reinterpret_cast<const RefitQuad*>(vertices) + slot_vtx[(size_t)first + j];
        for (int k = 0; k < 3; ++k) {
            const RefitQuad p = v[k];
            if (j == 0 && k == 0) { a.b[0] = a.b[1] = p.x; a.b[2] = a.b[3] = p.y; a.b[4] = a.b[5] = p.z; }
            else refit_merge(a, p.x, p.x, p.y, p.y, p.z, p.z);
        }
    }
    return a;
}

// the inner rule: the box of child 0 of a pair, child 1's merged into it.  q = the three 16-byte quarters of NodePair::b
PT_REFIT_HD RefitBox refit_union(const RefitQuad q[3]) {
    RefitBox a{{q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y}};
    refit_merge(a, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w);
    return a;
}

// pair k: the boxes of its two children (a leaf's from the vertices, an inner child's from the child's pair, which a deeper level has
// written already) into NodePair::b as three 16-byte stores; meta is read, never written.  Pair 0 also leaves the root's box in root6
PT_REFIT_HD void refit_pair(NodePair* pairs, uint32_t k, const float* vertices, const uint32_t* slot_vtx, float* root6) {
    RefitQuad* me = reinterpret_cast<RefitQuad*>(pairs + k);
    const RefitMeta meta = *reinterpret_cast<const RefitMeta*>(me + 3);
    const RefitQuad old[3] = {me[0], me[1], me[2]};
    const RefitBox old_box[2] = {{{old[0].x, old[0].y, old[0].z, old[0].w, old[1].x, old[1].y}}, {{old[1].z, old[1].w, old[2].x, old[2].y, old[2].z, old[2].w}}};
    RefitBox c[2];
    for (int ch = 0; ch < 2; ++ch) {
        const uint32_t a = meta.m[2 * ch], n = meta.m[2 * ch + 1];
        if (n == 0xFFFFFFFFu) {
            const RefitQuad* cq = reinterpret_cast<const RefitQuad*>(pairs + a);
            const RefitQuad q[3] = {cq[0], cq[1], cq[2]};
            c[ch] = refit_union(q);
        } else {
            c[ch] = refit_leaf_box(vertices, slot_vtx, a, n, old_box[ch]);           // (an empty leaf keeps the box it was uploaded with)
        }
    }
    const RefitQuad q[3] = {RefitQuad{c[0].b[0], c[0].b[1], c[0].b[2], c[0].b[3]}, RefitQuad{c[0].b[4], c[0].b[5], c[1].b[0], c[1].b[1]},
                            RefitQuad{c[1].b[2], c[1].b[3], c[1].b[4], c[1].b[5]}};
    me[0] = q[0]; me[1] = q[1]; me[2] = q[2];
    if (k == 0) {
        const RefitBox r = refit_union(q);
        for (int j = 0; j < 6; ++j) root6[j] = r.b[j];
    }
}

// a tree whose root is a leaf: the leaf rule over the root's slots into root6 (which holds the uploaded box on entry: an empty root keeps it)
PT_REFIT_HD void refit_root_leaf(const float* vertices, const uint32_t* slot_vtx, uint32_t first, uint32_t count, float* root6) {
    RefitBox keep;
    for (int j = 0; j < 6; ++j) keep.b[j] = root6[j];
    const RefitBox r = refit_leaf_box(vertices, slot_vtx, first, count, keep);
    for (int j = 0; j < 6; ++j) root6[j] = r.b[j];
}

}  // namespace prt
