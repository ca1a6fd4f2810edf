// pt_prims.hip -- prt_update_primitives on the device (prt.h): the prt_mesh records of the moved spheres, SDF primitives and quads into staging
// tables of DevSphere / DevSdf / DevQuad, by the body of pt_prims.h (pack_scene's expressions; pack_quad of pt_layout.h).  One lane per
// record: five 16-byte loads and a byte of the types table in, one to five 16-byte stores out.  No LDS, no atomics, no scratch, no waits
// between workgroups.
#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_prims.h"

namespace prt {

// a refused record sets the flag word (a plain store of 1: every lane that stores writes the same value)
__global__ __launch_bounds__(256) void prims_pack_kernel(const void* __restrict__ meshes, uint32_t count, uint32_t n_spheres, uint32_t n_sdfs,
                                                         const uint8_t* __restrict__ types, DevSphere* __restrict__ spheres,
                                                         DevSdf* __restrict__ sdfs, DevQuad* __restrict__ quads, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if (prims_pack(meshes, i, n_spheres, n_sdfs, types, spheres, sdfs, quads)) *flag = 1u;
}

void launch_prims_pack(const void* meshes, uint32_t count, uint32_t n_spheres, uint32_t n_sdfs, const uint8_t* types, DevSphere* spheres,
                       DevSdf* sdfs, DevQuad* quads, uint32_t* flag, hipStream_t stream) {
    if (!count) return;
    hipLaunchKernelGGL(prims_pack_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, meshes, count, n_spheres, n_sdfs, types, spheres, sdfs,
                       quads, flag);
}

}  // namespace prt
