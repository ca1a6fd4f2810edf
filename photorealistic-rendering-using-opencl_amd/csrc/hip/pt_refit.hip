// pt_refit.hip -- prt_update_vertices on the device (prt.h): new vertices into the triangle records and the boxes of the uploaded tree, its
// topology kept.  Bandwidth-bound streaming kernels around the bodies of pt_refit.h: no LDS, no atomics, no waits between workgroups.  The
// boxes go bottom-up with ONE LAUNCH PER LEVEL of pairs, deepest first: a level reads only what launches that have ended wrote.
#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_refit.h"

namespace prt {

// one lane per vertex: a non-finite x, y or z sets the flag word (a plain store of 1: every lane that stores writes the same value)
__global__ __launch_bounds__(256) void refit_check_kernel(const float* __restrict__ vertices, size_t n_vertices, uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vertices) return;
    if (!refit_vertex_finite(vertices, i)) *flag = 1u;
}

// one lane per slot
__global__ __launch_bounds__(256) void refit_tri_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                        const uint32_t* __restrict__ slot_vtx, size_t n_slots,
                                                        TriGeom* __restrict__ tri_geom, TriNrm* __restrict__ tri_nrm) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slots) return;
    refit_tri(vertices, normals, slot_vtx, s, tri_geom, tri_nrm);
}

// one lane per pair of one level: level_pairs[0 .. n) are the level's pair indices.  (pairs is read and written: children and parents are
// different records, no __restrict__)
__global__ __launch_bounds__(256) void refit_level_kernel(NodePair* pairs, const uint32_t* __restrict__ level_pairs, uint32_t n,
                                                          const float* __restrict__ vertices, const uint32_t* __restrict__ slot_vtx,
                                                          float* root6) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    refit_pair(pairs, level_pairs[i], vertices, slot_vtx, root6);
}

// a leaf root: one lane
__global__ __launch_bounds__(64) void refit_root_leaf_kernel(const float* __restrict__ vertices, const uint32_t* __restrict__ slot_vtx,
                                                             uint32_t first, uint32_t count, float* root6) {
    if (blockIdx.x == 0 && threadIdx.x == 0) refit_root_leaf(vertices, slot_vtx, first, count, root6);
}

void launch_refit_check(const float* vertices, size_t n_vertices, uint32_t* flag, hipStream_t stream) {
    if (!n_vertices) return;
    hipLaunchKernelGGL(refit_check_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, stream, vertices, n_vertices, flag);
}

void launch_refit(const RefitTables& t, const float* vertices, const float* normals, NodePair* pairs, TriGeom* tri_geom, TriNrm* tri_nrm,
                  float* root6, hipStream_t stream) {
    if (t.n_slots)
        hipLaunchKernelGGL(refit_tri_kernel, dim3((unsigned)((t.n_slots + 255) / 256)), dim3(256), 0, stream, vertices, normals, t.slot_vtx,
                           t.n_slots, tri_geom, tri_nrm);
    if (t.root_is_leaf) {
        hipLaunchKernelGGL(refit_root_leaf_kernel, dim3(1), dim3(64), 0, stream, vertices, t.slot_vtx, t.root_leaf_first, t.root_leaf_count, root6);
        return;
    }
    for (uint32_t l = t.n_levels; l-- > 0;) {
        const uint32_t first = t.level_first[l], n = t.level_first[l + 1] - first;
        if (!n) continue;
        hipLaunchKernelGGL(refit_level_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, pairs, t.level_pairs + first, n, vertices, t.slot_vtx,
                           root6);
    }
}

}  // namespace prt
