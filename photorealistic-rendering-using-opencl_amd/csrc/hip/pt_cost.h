// pt_cost.h -- the bodies of the tree-cost kernels (pt_cost.hip; prt.h prt_bvh_cost): the SAH cost of the current tree from its NodePair table
// and the root's box.  Plain pointers and __host__ __device__ inline functions only, so that a host harness (tests/emu/cost_emu.cpp) runs the
// same code serially.  f64 multiplies and adds as written, no contraction (build.py: -ffp-contract=off); one f64 division at the very end.
// The sum has ONE shape -- the complete binary tree over the pair index, the terms padded with +0.0 to a power of two -- so that no block
// size, grid size or schedule can change a bit of it: cost_level below, applied until one value is left, IS that tree, and what a block of
// the device reduces is a sub-tree of it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_refit.h"

#if defined(__HIPCC__)
#define PT_COST_HD __host__ __device__ inline
#else
#define PT_COST_HD inline
#endif

namespace prt {

// terms a block reduces: a power of two (a block's partial is then one node of the tree, 8 levels up)
constexpr uint32_t PT_COST_BLOCK = 256u;

// the area of a box given as the six floats of a NodePair child: min_x max_x min_y max_y min_z max_z.  max(d, 0) in its comparison form
PT_COST_HD double cost_area(const float* b) {
    const double ex = (double)b[1] - (double)b[0], ey = (double)b[3] - (double)b[2], ez = (double)b[5] - (double)b[4];
    const double dx = ex > 0.0 ? ex : 0.0, dy = ey > 0.0 ? ey : 0.0, dz = ez > 0.0 ? ez : 0.0;
    return 2.0 * ((dx * dy + dy * dz) + dz * dx);
}

// what one child weighs: an inner child its area, a leaf its area times its primitive count, an empty leaf +0 whatever its box
PT_COST_HD double cost_child(const float* b, uint32_t count) {
    if (count == 0xFFFFFFFFu) return 1.0 * cost_area(b);
    if (count == 0u) return 0.0;
    return (double)count * cost_area(b);
}

// the term of one pair from its four 16-byte quarters: q = NodePair::b, meta = NodePair::meta
PT_COST_HD double cost_pair_term(const RefitQuad q[3], const RefitMeta& meta) {
    const float b0[6] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y}, b1[6] = {q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
    return cost_child(b0, meta.m[1]) + cost_child(b1, meta.m[3]);
}

// the term of pair k of a table, as four 16-byte loads
PT_COST_HD double cost_term(const NodePair* pairs, size_t k) {
    const RefitQuad* me = reinterpret_cast<const RefitQuad*>(pairs + k);
    const RefitQuad q[3] = {me[0], me[1], me[2]};
    const RefitMeta meta = *reinterpret_cast<const RefitMeta*>(me + 3);
    return cost_pair_term(q, meta);
}

// one node of the pairwise tree
PT_COST_HD double cost_add(double left, double right) { return left + right; }

// one level of the tree: out[i] = in[2i] + in[2i + 1] for i < ceil(n / 2), an entry past n read as +0.0
PT_COST_HD void cost_level(const double* in, size_t n, double* out, size_t i) {
    const double left = in[2 * i], right = 2 * i + 1 < n ? in[2 * i + 1] : 0.0;
    out[i] = cost_add(left, right);
}

// the cost of a tree with an inner root from the sum S of its terms and pair 0 (the root's box: the union rule of the refit over pair 0)
PT_COST_HD double cost_inner_root(const NodePair* pairs, double S) {
    const RefitQuad* me = reinterpret_cast<const RefitQuad*>(pairs);
    const RefitQuad q[3] = {me[0], me[1], me[2]};
    const RefitBox r = refit_union(q);
    const double a = cost_area(r.b);
    return (a + S) / a;
}

// ... and of a tree whose root is a leaf of `count` triangles with the box root6
PT_COST_HD double cost_leaf_root(const float* root6, uint32_t count) {
    const double a = cost_area(root6);
    return cost_child(root6, count) / a;
}

}  // namespace prt
