// pt_pose.hip -- the mesh posed on the device from the frame's bone matrices (prt.h prt_set_skin / prt_pose): one launch around the body of
// pt_pose.h, in front of the refit's or the rebuild's own path.  One lane per corner, wave64, blocks of 256.  The lane streams its rest
// vertex, rest normal and weights as 16-byte loads, its four indices as one 8-byte load, and stores two float4: 88 bytes per corner with
// normals, 56 without.  The matrix table is the only access at a per-lane index: three 16-byte loads per influence with a non-zero weight,
// from global memory through the vector cache (pt_pose.h says why it is not staged in LDS).  No LDS, no scratch, no atomics, nothing
// between lanes: the result depends on the skin and the matrices only, whatever the launch shape.
#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_pose.h"

namespace prt {

__global__ __launch_bounds__(256) void pose_kernel(const float* __restrict__ rest_v, const float* __restrict__ rest_n,
                                                   const uint16_t* __restrict__ bone_index, const float* __restrict__ bone_weight,
                                                   const float* __restrict__ matrices, uint32_t n_corners, float* __restrict__ out_v,
                                                   float* __restrict__ out_n) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    pose_corner(rest_v, rest_n, bone_index, bone_weight, matrices, c, out_v, out_n);
}

void launch_pose(const PoseTables& t, const float* matrices, float* out_v, float* out_n, hipStream_t stream) {
    if (!t.n_tris) return;
    const uint32_t n_corners = 3u * t.n_tris;                   // (prt_set_skin: T <= PRT_MAX_TRIANGLE_SLOTS, so 3T fits)
    hipLaunchKernelGGL(pose_kernel, dim3((n_corners + 255u) / 256u), dim3(256), 0, stream, t.rest_v, t.rest_n, t.bone_index, t.bone_weight, matrices,
                       n_corners, out_v, t.rest_n ? out_n : nullptr);
}

}  // namespace prt
