// pt_morph.hip -- the mesh morphed on the device from the frame's target weights (prt.h prt_set_morph_targets / prt_morph /
// prt_pose_morphed): one launch around a body of pt_morph.h, in front of the refit's or the rebuild's own path.  One lane per corner, wave64,
// blocks of 256.  The lane streams its base vertex and base normal as 16-byte loads and its two table offsets, walks its entries -- one
// 16-byte record each, and one more with normals; consecutive corners own consecutive records --, reads each entry's weight from global
// memory through the vector cache, and stores two float4.  The fused kernel goes on with the pose of pt_pose.h over the morphed values in
// registers: the morphed rest pose never goes to memory.  The trip count differs per lane: a wave runs as long as its corner with the most
// entries.  No LDS, no scratch, no atomics, nothing between lanes: the result depends on the set and the weights only, whatever the launch
// shape.  A set under PRT_MORPH_LAYOUT_PLANES runs the two plane kernels below instead, one wave per block of 64 corners.
#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_morph.h"

namespace prt {

__global__ __launch_bounds__(256) void morph_kernel(const float* __restrict__ base_v, const float* __restrict__ base_n,
                                                    const uint32_t* __restrict__ offset, const float* __restrict__ entry_p,
                                                    const float* __restrict__ entry_n, const float* __restrict__ weights, uint32_t n_corners,
                                                    float* __restrict__ out_v, float* __restrict__ out_n) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    morph_corner(base_v, base_n, offset, entry_p, entry_n, weights, c, out_v, out_n);
}

__global__ __launch_bounds__(256) void pose_morphed_kernel(const float* __restrict__ base_v, const float* __restrict__ base_n,
                                                           const uint32_t* __restrict__ offset, const float* __restrict__ entry_p,
                                                           const float* __restrict__ entry_n, const float* __restrict__ weights,
                                                           const uint16_t* __restrict__ bone_index, const float* __restrict__ bone_weight,
                                                           const float* __restrict__ matrices, uint32_t n_corners, float* __restrict__ out_v,
                                                           float* __restrict__ out_n) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    pose_morphed_corner(base_v, base_n, offset, entry_p, entry_n, weights, bone_index, bone_weight, matrices, c, out_v, out_n);
}

// The plane table (pt_morph.h): one wave per block of 64 corners, four blocks per workgroup.  The block's number is made of blockIdx and the
// first lane's wave number, so the compiler knows it to be the same in every lane: block_first, the plane's head and its weight are scalar
// loads, and a plane under a zero weight is skipped by a scalar branch before any of its rows is asked for.  A row is 256 contiguous bytes
// for the 64 lanes.  Lanes past 3T leave before the loop; the planes of the ragged block still have 64 lanes
__global__ __launch_bounds__(256) void morph_planes_kernel(const float* __restrict__ base_v, const float* __restrict__ base_n,
                                                           const uint32_t* __restrict__ block_first, const MorphPlaneHead* __restrict__ plane_head,
                                                           const float* __restrict__ plane_p, const float* __restrict__ plane_n,
                                                           const float* __restrict__ weights, uint32_t n_corners, float* __restrict__ out_v,
                                                           float* __restrict__ out_n) {
    const uint32_t b = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = threadIdx.x & 63u;
    if ((size_t)b * 64 + l >= n_corners) return;
    morph_planes_corner(base_v, base_n, block_first, plane_head, plane_p, plane_n, weights, b, l, out_v, out_n);
}

__global__ __launch_bounds__(256) void pose_morphed_planes_kernel(const float* __restrict__ base_v, const float* __restrict__ base_n,
                                                                  const uint32_t* __restrict__ block_first,
                                                                  const MorphPlaneHead* __restrict__ plane_head, const float* __restrict__ plane_p,
                                                                  const float* __restrict__ plane_n, const float* __restrict__ weights,
                                                                  const uint16_t* __restrict__ bone_index, const float* __restrict__ bone_weight,
                                                                  const float* __restrict__ matrices, uint32_t n_corners, float* __restrict__ out_v,
                                                                  float* __restrict__ out_n) {
    const uint32_t b = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = threadIdx.x & 63u;
    if ((size_t)b * 64 + l >= n_corners) return;
    pose_morphed_planes_corner(base_v, base_n, block_first, plane_head, plane_p, plane_n, weights, bone_index, bone_weight, matrices, b, l, out_v,
                               out_n);
}

void launch_morph(const MorphTables& t, const float* weights, float* out_v, float* out_n, hipStream_t stream) {
    if (!t.n_tris) return;
    const uint32_t n_corners = 3u * t.n_tris;                   // (prt_set_morph_targets: T <= PRT_MAX_TRIANGLE_SLOTS, so 3T fits)
    if (t.planes) {
        hipLaunchKernelGGL(morph_planes_kernel, dim3((n_corners + 255u) / 256u), dim3(256), 0, stream, t.base_v, t.base_n, t.block_first,
                           static_cast<const MorphPlaneHead*>(t.plane_head), t.plane_p, t.plane_n, weights, n_corners, out_v, t.base_n ? out_n : nullptr);
        return;
    }
    hipLaunchKernelGGL(morph_kernel, dim3((n_corners + 255u) / 256u), dim3(256), 0, stream, t.base_v, t.base_n, t.offset, t.entry_p, t.entry_n, weights,
                       n_corners, out_v, t.base_n ? out_n : nullptr);
}

void launch_pose_morphed(const MorphTables& t, const PoseTables& skin, const float* matrices, const float* weights, float* out_v, float* out_n,
                         hipStream_t stream) {
    if (!t.n_tris) return;
    const uint32_t n_corners = 3u * t.n_tris;
    if (t.planes) {
        hipLaunchKernelGGL(pose_morphed_planes_kernel, dim3((n_corners + 255u) / 256u), dim3(256), 0, stream, t.base_v, t.base_n, t.block_first,
                           static_cast<const MorphPlaneHead*>(t.plane_head), t.plane_p, t.plane_n, weights, skin.bone_index, skin.bone_weight, matrices,
                           n_corners, out_v, t.base_n ? out_n : nullptr);
        return;
    }
    hipLaunchKernelGGL(pose_morphed_kernel, dim3((n_corners + 255u) / 256u), dim3(256), 0, stream, t.base_v, t.base_n, t.offset, t.entry_p, t.entry_n,
                       weights, skin.bone_index, skin.bone_weight, matrices, n_corners, out_v, t.base_n ? out_n : nullptr);
}

}  // namespace prt
