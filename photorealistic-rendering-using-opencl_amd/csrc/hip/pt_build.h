// pt_build.h -- the bodies of the build kernels (pt_build.hip; prt.h prt_rebuild_bvh): new vertices -> a Morton-order tree over all T triangles
// in the tables a refit reads (NodePair::meta, slot_vtx, level_pairs, level_first); the records and the boxes are then pt_refit.h's.  Plain
// pointers and __host__ __device__ inline functions only, so that a host harness (tests/emu/build_emu.cpp) runs the same code serially.  f32
// operations, no contraction (build.py: -ffp-contract=off).  The rule numbers are those of prt.h.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "pt_layout.h"
#include "pt_refit.h"

#if defined(__HIPCC__)
#define PT_BUILD_HD __host__ __device__ inline
#else
#define PT_BUILD_HD inline
#endif

namespace prt {

#define PT_BUILD_NONE 0xFFFFFFFFu
#define PT_BUILD_DEFAULT_LEAF 4u        // max_leaf == 0 (prt.h): the leaf size whose tree of the 871 k-triangle mesh renders fastest (DESIGN.md s4 "Rebuild")
#define PT_BUILD_NO_DEPTH 64u          // the depth field of a range that is no pair (a pair's depth is at most 62)

// rule 2: what the codes are scaled by
struct alignas(16) BuildExtent { float lo[3]; float pad0; float scale[3]; float pad1; };
// one inner node of the radix tree over the sorted keys: the positions first .. last it covers, split behind `split`
struct alignas(16) BuildNode { uint32_t first, last, split, pad; };
// what the host reads back in one copy: pairs, levels of pairs, most pairs with two inner children on a path, then level_first[0 .. levels]
struct BuildHeader { uint32_t n_pairs, n_levels, max_two, pad; uint32_t level_first[68]; };

// rule 1: the triangle's box by the leaf rule over its three vertices, the centre per axis lo * 0.5f + hi * 0.5f
PT_BUILD_HD void build_centre(const float* vertices, uint32_t tri, float c[3]) {
    const RefitQuad* v = reinterpret_cast<const RefitQuad*>(vertices) + 3 * (size_t)tri;
    const RefitQuad p0 = v[0], p1 = v[1], p2 = v[2];
    RefitBox a{{p0.x, p0.x, p0.y, p0.y, p0.z, p0.z}};
    refit_merge(a, p1.x, p1.x, p1.y, p1.y, p1.z, p1.z);
    refit_merge(a, p2.x, p2.x, p2.y, p2.y, p2.z, p2.z);
    for (int k = 0; k < 3; ++k) c[k] = a.b[2 * k] * 0.5f + a.b[2 * k + 1] * 0.5f;
}

// rule 2: lo / hi of the centres merge by comparisons (the values are finite: any order gives the same values up to the sign of a zero) ...
PT_BUILD_HD void build_extent_merge(float lo[3], float hi[3], const float lo2[3], const float hi2[3]) {
    for (int k = 0; k < 3; ++k) { lo[k] = lo2[k] < lo[k] ? lo2[k] : lo[k]; hi[k] = hi2[k] > hi[k] ? hi2[k] : hi[k]; }
}
// ... and + 0.0f takes that sign out
PT_BUILD_HD BuildExtent build_extent_finish(const float lo[3], const float hi[3]) {
    BuildExtent e;
    e.pad0 = e.pad1 = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float l = lo[k] + 0.0f, h = hi[k] + 0.0f;
        e.lo[k] = l;
        e.scale[k] = h > l ? 1024.0f / (h - l) : 0.0f;
    }
    return e;
}

PT_BUILD_HD uint32_t build_spread3(uint32_t q) {       // 10 bits -> every third bit of 30
    q = (q | (q << 16)) & 0x030000FFu;
    q = (q | (q << 8)) & 0x0300F00Fu;
    q = (q | (q << 4)) & 0x030C30C3u;
    q = (q | (q << 2)) & 0x09249249u;
    return q;
}

// rules 3 and 4: the key of triangle `tri`
PT_BUILD_HD uint64_t build_key(const float* vertices, uint32_t tri, const BuildExtent& e) {
    float c[3];
    build_centre(vertices, tri, c);
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float t = (c[k] - e.lo[k]) * e.scale[k];
        q[k] = (uint32_t)(t < 1023.0f ? t : 1023.0f);
    }
    const uint32_t code = (build_spread3(q[0]) << 2) | (build_spread3(q[1]) << 1) | build_spread3(q[2]);
    return ((uint64_t)code << 32) | tri;
}

// length of the common prefix of keys i and j (distinct keys: at most 63), -1 for a j outside 0 .. n - 1
PT_BUILD_HD int build_delta(const uint64_t* keys, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(keys[i] ^ keys[j]);
}

// rule 5: inner node i (0 .. n - 2) of the binary radix tree over n >= 2 sorted distinct keys (Karras 2012): node 0 is the root; an inner
// child is the node numbered like the end of its range that touches the split.  Writes the node and the parent of its inner children
PT_BUILD_HD void build_node(const uint64_t* keys, uint32_t n_keys, uint32_t i_, BuildNode* nodes, uint32_t* parent) {
    const int64_t n = n_keys, i = i_;
    const int d = build_delta(keys, n, i, i + 1) > build_delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = build_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (build_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (build_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = build_delta(keys, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (build_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t a = i < j ? i : j, b = i < j ? j : i;
    nodes[i] = BuildNode{(uint32_t)a, (uint32_t)b, (uint32_t)g, 0u};
    if (i == 0) parent[0] = PT_BUILD_NONE;
    if (g > a) parent[g] = (uint32_t)i;
    if (g + 1 < b) parent[g + 1] = (uint32_t)i;
}

PT_BUILD_HD bool build_two_inner(const BuildNode& nd, uint32_t max_leaf) { return nd.split - nd.first + 1u > max_leaf && nd.last - nd.split > max_leaf; }

// rules 5 and 6: the sort key of inner node i -- (depth, first) of a range of more than max_leaf triangles (a pair: every range above it is
// one too), (PT_BUILD_NO_DEPTH, first) of any other.  *two = the pair's count of itself and the pairs above it with two inner children
PT_BUILD_HD uint64_t build_pair_key(const BuildNode* nodes, const uint32_t* parent, uint32_t i, uint32_t max_leaf, uint32_t* two) {
    const BuildNode me = nodes[i];
    *two = 0;
    if (me.last - me.first + 1u <= max_leaf) return ((uint64_t)PT_BUILD_NO_DEPTH << 32) | me.first;
    uint32_t depth = 0, cnt = 0, j = i;
    for (;;) {                                          // at most 62 steps: a level splits on a lower bit of the 62-bit key
        cnt += build_two_inner(nodes[j], max_leaf) ? 1u : 0u;
        const uint32_t p = parent[j];
        if (p == PT_BUILD_NONE) break;
        ++depth;
        j = p;
    }
    *two = cnt;
    return ((uint64_t)depth << 32) | me.first;
}

// position k of the sorted pair keys (n of them, n = inner nodes; keys[k] >> 32 < PT_BUILD_NO_DEPTH: pair k is node order[k]): the pair's
// number into pair_of, the triangles of its leaf children into leaf_tris, and, where k starts a level or ends the pairs, the header's entries
PT_BUILD_HD void build_number(const uint64_t* keys, const uint32_t* order, uint32_t n, uint32_t k, const BuildNode* nodes, uint32_t max_leaf,
                              uint32_t* pair_of, uint32_t* leaf_tris, BuildHeader* hdr) {
    const uint32_t dk = (uint32_t)(keys[k] >> 32);
    if (dk >= PT_BUILD_NO_DEPTH) { leaf_tris[k] = 0; return; }
    const BuildNode nd = nodes[order[k]];
    pair_of[order[k]] = k;
    const uint32_t n0 = nd.split - nd.first + 1u, n1 = nd.last - nd.split;
    leaf_tris[k] = (n0 <= max_leaf ? n0 : 0u) + (n1 <= max_leaf ? n1 : 0u);
    if (k == 0 || (uint32_t)(keys[k - 1] >> 32) != dk) hdr->level_first[dk] = k;
    if (k + 1 == n || (uint32_t)(keys[k + 1] >> 32) >= PT_BUILD_NO_DEPTH) { hdr->level_first[dk + 1] = k + 1; hdr->n_pairs = k + 1; hdr->n_levels = dk + 1; }
}

// rules 6 and 7: pair k -- NodePair::meta (the boxes zeroed: the refit writes them), the slots of its leaf children from slot_base[k] on
// (the exclusive sum of leaf_tris), left leaf first, triangles in sorted order, and the identity entry of level_pairs
PT_BUILD_HD void build_pair(const uint64_t* pair_keys, const uint32_t* order, uint32_t k, const BuildNode* nodes, const uint32_t* pair_of,
                            const uint32_t* slot_base, const uint64_t* tri_keys, uint32_t max_leaf, NodePair* pairs, uint32_t* slot_vtx,
                            uint32_t* level_pairs) {
    if ((uint32_t)(pair_keys[k] >> 32) >= PT_BUILD_NO_DEPTH) return;
    const BuildNode nd = nodes[order[k]];
    const uint32_t first[2] = {nd.first, nd.split + 1u}, last[2] = {nd.split, nd.last};
    RefitMeta m;
    uint32_t slot = slot_base[k];
    for (int ch = 0; ch < 2; ++ch) {
        const uint32_t cnt = last[ch] - first[ch] + 1u;
        if (cnt > max_leaf) {
            m.m[2 * ch] = pair_of[ch == 0 ? nd.split : nd.split + 1u];
            m.m[2 * ch + 1] = 0xFFFFFFFFu;
        } else {
            m.m[2 * ch] = slot;
            m.m[2 * ch + 1] = cnt;
            for (uint32_t j = 0; j < cnt; ++j) slot_vtx[(size_t)slot + j] = (uint32_t)tri_keys[first[ch] + j] * 3u;
            slot += cnt;
        }
    }
    RefitQuad* me = reinterpret_cast<RefitQuad*>(pairs + k);
    me[0] = me[1] = me[2] = RefitQuad{0.0f, 0.0f, 0.0f, 0.0f};
    *reinterpret_cast<RefitMeta*>(me + 3) = m;
    level_pairs[k] = k;
}

// a leaf root (T <= max_leaf): slot s holds the triangle of sorted position s
PT_BUILD_HD void build_root_slot(const uint64_t* tri_keys, uint32_t s, uint32_t* slot_vtx) { slot_vtx[s] = (uint32_t)tri_keys[s] * 3u; }

// "old slot of triangle" (prt.h: what a rebuild carries over): old slot s names its triangle; where leaves shared one any writer wins
PT_BUILD_HD void build_old_slot(const uint32_t* old_slot_vtx, uint32_t s, uint32_t* old_slot) { old_slot[old_slot_vtx[s] / 3u] = s; }

// new slot s: TriNrm from the triangle's old slot (carry_nrm; the caller has checked that every triangle has one), and the motion snapshot
// (prev_new non-null): the old record of the triangle -- prev_old is the pending snapshot or the records before the rebuild, in the old slot
// order -- or, for a triangle the old tree did not hold, its new record (no motion)
PT_BUILD_HD void build_carry(const uint32_t* slot_vtx, uint32_t s, const uint32_t* old_slot, bool carry_nrm, const TriNrm* nrm_old, TriNrm* nrm_new,
                             const TriGeom* prev_old, const TriGeom* geom_new, TriGeom* prev_new) {
    const uint32_t os = old_slot[slot_vtx[s] / 3u];
    if (carry_nrm && os != PT_BUILD_NONE) {
        const RefitQuad* a = reinterpret_cast<const RefitQuad*>(nrm_old + os);
        RefitQuad* b = reinterpret_cast<RefitQuad*>(nrm_new + s);
        const RefitQuad q0 = a[0], q1 = a[1], q2 = a[2];
        b[0] = q0; b[1] = q1; b[2] = q2;
    }
    if (prev_new) {
        const RefitQuad* a = os != PT_BUILD_NONE ? reinterpret_cast<const RefitQuad*>(prev_old + os) : reinterpret_cast<const RefitQuad*>(geom_new + s);
        RefitQuad* b = reinterpret_cast<RefitQuad*>(prev_new + s);
        const RefitQuad q0 = a[0], q1 = a[1], q2 = a[2];
        b[0] = q0; b[1] = q1; b[2] = q2;
    }
}

}  // namespace prt
