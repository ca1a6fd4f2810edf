// pt_normals.hip -- smooth shading normals regenerated on the device from new vertices (prt.h prt_set_smooth_normals): two launches around the
// bodies of pt_normals.h, in front of the refit's record pass.  No LDS, no atomics, no waits between workgroups: the face kernel streams
// (three 16-byte loads and one or two 16-byte stores per lane), the corner kernel gathers one 16-byte face record per member of its group
// -- T records of 16 bytes, which neighbouring corners share and the caches hold -- and stores one float4.  The sum of a corner runs in
// the table's order whatever the launch shape: the result depends on the vertices and the topology only.
#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_normals.h"

namespace prt {

// one lane per triangle
__global__ __launch_bounds__(256) void normals_face_kernel(const float* __restrict__ vertices, uint32_t n_tris, RefitQuad* __restrict__ face_f,
                                                           RefitQuad* __restrict__ face_r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tris) return;
    normals_face(vertices, i, face_f, face_r);
}

// one lane per corner
__global__ __launch_bounds__(256) void normals_corner_kernel(const uint32_t* __restrict__ corner_group, const uint32_t* __restrict__ group_first,
                                                             const uint32_t* __restrict__ member_face, const RefitQuad* __restrict__ face_f,
                                                             const RefitQuad* __restrict__ face_r, float crease_cos, uint32_t n_corners,
                                                             float* __restrict__ normals) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    normals_corner(corner_group, group_first, member_face, face_f, face_r, crease_cos, (uint32_t)c, normals);
}

void launch_smooth_normals(const SmoothTables& t, const float* vertices, float* normals, hipStream_t stream) {
    if (!t.n_tris) return;
    RefitQuad* face_f = static_cast<RefitQuad*>(t.face_f);
    RefitQuad* face_r = static_cast<RefitQuad*>(t.face_r);
    const uint32_t n_corners = 3u * t.n_tris;                   // (prt_set_smooth_normals: T <= PRT_MAX_TRIANGLE_SLOTS, so 3T fits)
    hipLaunchKernelGGL(normals_face_kernel, dim3((t.n_tris + 255u) / 256u), dim3(256), 0, stream, vertices, t.n_tris, face_f, face_r);
    hipLaunchKernelGGL(normals_corner_kernel, dim3((n_corners + 255u) / 256u), dim3(256), 0, stream, t.corner_group, t.group_first, t.member_face,
                       face_f, face_r, t.crease_cos, n_corners, normals);
}

}  // namespace prt
