// pt_cost.hip -- prt_bvh_cost on the device (prt.h): the SAH cost of the current tree, summed in the one shape pt_cost.h fixes.  A block of
// PT_COST_BLOCK lanes reduces its run of PT_COST_BLOCK consecutive terms in adjacent-pair order -- shuffle-down by 1, 2, 4, ..., 32 inside a
// wave, the four waves' values through LDS -- and writes ONE f64 partial: node `blockIdx` of the tree, 8 levels up.  The partials are reduced
// the same way by the next launch, until one value is left; the block that produces it also forms the cost.  No atomics, no hand-off
// between workgroups inside a launch: a level reads only what a launch that has ended wrote.
#include <hip/hip_runtime.h>

#include "pt_cost.h"
#include "pt_launch.h"

namespace prt {

static_assert(PT_COST_BLOCK == 256u, "cost_block_sum: four waves of 64 lanes");

// the sum of the block's PT_COST_BLOCK values `t` (one per lane) as the complete binary tree over the lane index; valid in lane 0
__device__ inline double cost_block_sum(double t, double* lds) {
    for (int off = 1; off < 64; off <<= 1) t = cost_add(t, __shfl_down(t, off, 64));      // lane i: the node over lanes i .. i + 2 off - 1
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = t;
    __syncthreads();
    return cost_add(cost_add(lds[0], lds[1]), cost_add(lds[2], lds[3]));
}

// level 0: one lane per pair, a lane past the table holds the padding's +0.0.  finish (the launch of one block only): S is complete -- the
// cost goes to out[0] instead of the partial
__global__ __launch_bounds__(PT_COST_BLOCK) void cost_terms_kernel(const NodePair* __restrict__ pairs, uint32_t n_pairs, double* __restrict__ out,
                                                                  int finish) {
    __shared__ double lds[4];
    const uint32_t k = blockIdx.x * PT_COST_BLOCK + threadIdx.x;
    const double S = cost_block_sum(k < n_pairs ? cost_term(pairs, k) : 0.0, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = finish ? cost_inner_root(pairs, S) : S;
}

// a further level: one lane per partial of the level below
__global__ __launch_bounds__(PT_COST_BLOCK) void cost_reduce_kernel(const double* __restrict__ in, uint32_t n, double* __restrict__ out,
                                                                   const NodePair* __restrict__ pairs, int finish) {
    __shared__ double lds[4];
    const uint32_t i = blockIdx.x * PT_COST_BLOCK + threadIdx.x;
    const double S = cost_block_sum(i < n ? in[i] : 0.0, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = finish ? cost_inner_root(pairs, S) : S;
}

// a tree whose root is a leaf: one lane.  root6 the root's box on the device, or null: `box`, as uploaded
__global__ __launch_bounds__(64) void cost_leaf_root_kernel(const float* __restrict__ root6, RefitBox box, uint32_t count, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (root6) for (int j = 0; j < 6; ++j) box.b[j] = root6[j];
    out[0] = cost_leaf_root(box.b, count);
}

size_t cost_work_doubles(uint32_t n_pairs) {
    size_t total = 0, n = n_pairs;
    do {
        n = (n + PT_COST_BLOCK - 1) / PT_COST_BLOCK;      // the partials of one level, each level behind the one below
        total += n;
    } while (n > 1);
    return total ? total : 1;                             // (a leaf root: the cost alone)
}

const double* launch_bvh_cost(const NodePair* pairs, uint32_t n_pairs, double* work, hipStream_t stream) {
    uint32_t n = (n_pairs + PT_COST_BLOCK - 1) / PT_COST_BLOCK;
    hipLaunchKernelGGL(cost_terms_kernel, dim3(n), dim3(PT_COST_BLOCK), 0, stream, pairs, n_pairs, work, n == 1 ? 1 : 0);
    while (n > 1) {
        const uint32_t blocks = (n + PT_COST_BLOCK - 1) / PT_COST_BLOCK;
        hipLaunchKernelGGL(cost_reduce_kernel, dim3(blocks), dim3(PT_COST_BLOCK), 0, stream, work, n, work + n, pairs, blocks == 1 ? 1 : 0);
        work += n;
        n = blocks;
    }
    return work;
}

void launch_bvh_cost_leaf_root(const float* root6, const float* host_root6, uint32_t count, double* work, hipStream_t stream) {
    RefitBox box;
    for (int j = 0; j < 6; ++j) box.b[j] = host_root6[j];
    hipLaunchKernelGGL(cost_leaf_root_kernel, dim3(1), dim3(64), 0, stream, root6, box, count, work);
}

}  // namespace prt
